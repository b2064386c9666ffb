"""Times the per-pixel variance and the variance-guided a-trous denoiser on one GPU.

    python scripts/bench_variance.py [--window 0.5] [--out profiles/variance/bench.jsonl] [--keep-trace DIR]

Two settings, each pair timed in the same run:
  c2   scene01, 1024x1024, the C2 camera, 1024 spp in chunks of 32 (wavefront, lean)
  qe   qe_scene01 read as tinyobj, 640x480, QuinEngine mode, 4 spp in chunks of 1
       (the viewer's 1-spp frame is a single chunk, which has no variance)
Per setting: mcpt_render_device against mcpt_render_var_device, and
mcpt_denoise_device against mcpt_denoise_var_device with their defaults
(5 iterations); the guided filter's time is also given as a ratio to the plain
filter's.  Every such figure is the median of device-event times over repeats
filling a window of at least --window seconds after a warm-up; the spread is
(max - min) / median.

The variance kernel alone is a fraction of a percent of its frame, below the
frame's spread, so it is not a difference of frame times: a child process runs
render_var_device under `rocprofv3 --kernel-trace` and the kernel's dispatches
are read from the trace (median and spread over --trace-frames dispatches per
setting).  The child's frames keep the setting's size, spp and chunk -- which
fix the kernel's work: K chunks, and how many units went through the tail-split
buffer -- at max_depth 0, so that the traced run stays short.  Achieved bytes/s
are given against the model of 2 x K x 16 B per pixel.
Prints one JSON line (and appends it to --out).
"""
import argparse
import csv
import dataclasses
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import montecarlopathtracer_amd as M  # noqa: E402


def timed(fn, window_s, min_reps=3, max_reps=2000):
    """median / spread of fn's device time: one warm-up, then repeats for >= window_s"""
    fn()
    torch.cuda.synchronize()
    times, total = [], 0.0
    while (total < window_s * 1e3 or len(times) < min_reps) and len(times) < max_reps:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1)
        times.append(t)
        total += t
    return summary(times)


def summary(times):
    times = sorted(times)
    med = times[len(times) // 2]
    return {"ms": round(med, 4), "spread": round((times[-1] - times[0]) / med, 4), "reps": len(times)}


def settings(c2_spp):
    """[(name, scene constructor, frame)] in the order the trace child runs them"""
    return [
        ("c2_1024x1024", lambda: M.Scene(M.ObjModel(M.scene_path("scene01"))),
         M.RenderParams.for_scene(1, width=1024, height=1024, spp=c2_spp, spp_chunk=32, pipeline="wavefront",
                                  lean=True)),
        ("qe_640x480", lambda: M.Scene(M.ObjModel(M.scene_path("qe_scene01"), flavor="tinyobj")),
         M.RenderParams.for_quinengine(seed=822569775, lean=True, spp=4, spp_chunk=1)),
    ]


def setting(scene, frame, window_s, iterations=5):
    W, H = frame.width, frame.height
    st = torch.cuda.current_stream().cuda_stream
    fb, var, ac, nd, out, scratch = (torch.zeros((H, W, 4), device="cuda") for _ in range(6))
    scene.reserve(frame)
    K = -(-frame.spp // frame.spp_chunk)
    res = {"width": W, "height": H, "spp": frame.spp, "chunk": frame.spp_chunk, "K": K, "pipeline": frame.pipeline}
    res["render"] = timed(lambda: scene.render_device(frame, fb.data_ptr(), st), window_s, min_reps=2)
    res["render_var"] = timed(lambda: scene.render_var_device(frame, fb.data_ptr(), var.data_ptr(), st), window_s,
                              min_reps=2)
    res["render_var"]["ratio_to_render"] = round(res["render_var"]["ms"] / res["render"]["ms"], 4)
    scene.render_aov_device(dataclasses.replace(frame, spp=4), ac.data_ptr(), nd.data_ptr(), st)
    gamma = frame.mode == "quinengine"
    res["denoise"] = timed(lambda: M.denoise_device(W, H, fb.data_ptr(), ac.data_ptr(), nd.data_ptr(), out.data_ptr(),
                                                    scratch.data_ptr(), st, gamma_space=gamma), window_s)
    d = timed(lambda: M.denoise_var_device(W, H, fb.data_ptr(), var.data_ptr(), ac.data_ptr(), nd.data_ptr(),
                                           out.data_ptr(), scratch.data_ptr(), st, gamma_space=gamma), window_s)
    d["iterations"] = iterations
    d["ratio_to_plain"] = round(d["ms"] / res["denoise"]["ms"], 4)
    d["GBps_vs_64B_floor"] = round(W * H * iterations * 64 / (d["ms"] * 1e-3) / 1e9, 1)
    res["denoise_var"] = d
    scene.stats()
    return res


def trace_child(c2_spp, frames):
    """render_var_device `frames` times per setting, cheap frames of the same partial-sum layout"""
    for _, make, frame in settings(c2_spp):
        scene = make()
        cheap = dataclasses.replace(frame, max_depth=0)
        fb, var = (torch.zeros((cheap.height, cheap.width, 4), device="cuda") for _ in range(2))
        for _ in range(frames + 1):                       # the first dispatch is the warm-up
            scene.render_var_device(cheap, fb.data_ptr(), var.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        scene.stats()
        del scene


def traced_variance_kernel(c2_spp, frames, keep, timeout_s=300):
    """{setting: median / spread of variance_kernel's dispatches} from a kernel trace, or an error note"""
    if not shutil.which("rocprofv3"):
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="mcpt_vartrace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--c2-spp", str(c2_spp), "--trace-frames", str(frames)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s)
        except subprocess.TimeoutExpired:
            return {"error": "traced run timed out"}
        if r.returncode != 0:
            return {"error": f"traced run failed ({r.returncode}): {r.stderr[-300:]}"}
        rows = []
        for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            if keep:
                os.makedirs(keep, exist_ok=True)
                shutil.copy(f, os.path.join(keep, os.path.basename(f)))
            with open(f) as fh:
                for row in csv.DictReader(fh):
                    if "variance_kernel" in row.get("Kernel_Name", ""):
                        rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
        rows.sort()
        names = [n for n, _, _ in settings(c2_spp)]
        if len(rows) != len(names) * (frames + 1):
            return {"error": f"{len(rows)} variance_kernel dispatches traced, expected {len(names) * (frames + 1)}"}
        res = {}
        for i, n in enumerate(names):
            mine = rows[i * (frames + 1) + 1:(i + 1) * (frames + 1)]
            res[n] = summary([(e - s) / 1e6 for s, e in mine])
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default="")
    ap.add_argument("--c2-spp", type=int, default=1024)
    ap.add_argument("--trace-frames", type=int, default=10)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--keep-trace", default="", help="directory that receives the raw kernel trace csv")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    if a.trace_child:
        trace_child(a.c2_spp, a.trace_frames)
        return
    line = {"bench": "variance", "device": torch.cuda.get_device_name(0), "window_s": a.window}
    for name, make, frame in settings(a.c2_spp):
        scene = make()
        line[name] = setting(scene, frame, a.window)
        del scene
    torch.cuda.synchronize()
    tr = traced_variance_kernel(a.c2_spp, a.trace_frames, a.keep_trace)
    for name, _, _ in settings(a.c2_spp):
        if name in tr:
            k = tr[name]
            r = line[name]
            k["model_bytes"] = 2 * r["K"] * 16 * r["width"] * r["height"]
            k["GBps_vs_model"] = round(k["model_bytes"] / (k["ms"] * 1e-3) / 1e9, 1)
            k["share_of_frame"] = round(k["ms"] / r["render"]["ms"], 6)
            r["variance_kernel"] = k
    if "error" in tr:
        line["variance_kernel_error"] = tr["error"]
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

"""Times variance-driven adaptive sampling (mcpt_render_adaptive_device) on one GPU.

    python scripts/bench_adaptive.py [--pipeline megakernel|wavefront] [--window 0.5]
                                     [--out profiles/adaptive/bench.jsonl] [--keep-trace DIR]

Setting: scene01 at the C2 camera, 1024x1024, megakernel (lean), --passes (16)
passes of --spp (64) samples in chunks of --chunk (8).  In one run:
  adaptive      the adaptive render at the default threshold (0.2, dilate 1)
  uniform       the chain of --passes uniform render_var_device calls (prev_count = j)
  one_render    one render_device of passes x spp samples in chunks of 32
  list_overhead force_list = 1 with min_passes = max_passes = 4 (every pixel through the
                pixel list in passes 1..3) against the 4-call uniform chain
Each is the median of device-event times around the whole call over repeats
filling a window of at least --window seconds after a warm-up; the spread is
(max - min) / median.  Rays come from the render's own counters (identical from
run to run), G rays/s = rays / median time.

Per pass: the active fraction (from the pass-count map), the rays (the counters
of adaptive renders cut at 1, 2, ... passes, differenced) and the kernel times
from a child process under `rocprofv3 --kernel-trace` (median over
--trace-frames renders): the pass's path kernel, and the selection (over,
count, scan, scatter) and merge kernels around it.  What the adaptive call
spends outside its kernels -- launches, and one 4-byte copy to pinned memory and
a stream wait per listed pass -- is given as the whole call's time less the
traced kernels', per listed pass.
--pipeline wavefront (mcpt_render_adaptive_ex_device; the record is
profiles/adaptive/bench_wf.jsonl): the same setting and the same four timings on
the wavefront -- list_overhead then prices the explicit queue 0 of a listed pass
against the implicit one, both sides rendering the same pixels -- plus, in the
same process, megakernel_adaptive: the megakernel's adaptive render of the same
params.  The traced child then gives, per listed pass, the kernel times of its
generate (wf_generate_list), its bounce-0 extend and shade (the first extend and
shade of each batch, by queue) and the rest (later bounces, cull, accumulate).
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
    return {"ms": round(med, 4), "spread": round((times[-1] - times[0]) / med, 4) if med else 0.0, "reps": len(times)}


def frame_of(a):
    return M.RenderParams.for_scene(1, width=a.size, height=a.size, spp=a.spp, spp_chunk=a.chunk, lean=True,
                                    pipeline=a.pipeline)


class Bufs:
    def __init__(self, frame):
        H, W = frame.height, frame.width
        self.fb, self.var = (torch.zeros((H, W, 4), device="cuda") for _ in range(2))
        self.cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream

    def adaptive(self, scene, frame, ap):
        # (the megakernel through the entry it always had; the general form honours the pipeline)
        entry = scene.render_adaptive_device if frame.pipeline == "megakernel" else scene.render_adaptive_ex_device
        entry(frame, ap, self.fb.data_ptr(), self.var.data_ptr(), self.cnt.data_ptr(), self.st)

    def uniform(self, scene, frame, passes):
        for j in range(passes):
            scene.render_var_device(dataclasses.replace(frame, spp_offset=j * frame.spp, prev_count=j),
                                    self.fb.data_ptr(), self.var.data_ptr(), self.st)


def with_rays(scene, res, fn):
    """res plus the rays of one run of fn and the rate at the median time"""
    scene.stats()
    fn()
    torch.cuda.synchronize()
    st = scene.stats()
    res["rays"] = st["rays"]
    res["renders"] = st["renders"]
    res["Grays_per_s"] = round(st["rays"] / (res["ms"] * 1e-3) / 1e9, 3)
    return res


def trace_child(a):
    """the adaptive render --trace-frames times (plus a warm-up)"""
    frame = frame_of(a)
    scene = M.Scene(M.ObjModel(M.scene_path("scene01")))
    b = Bufs(frame)
    for _ in range(a.trace_frames + 1):
        b.adaptive(scene, frame, M.adaptive_params(max_passes=a.passes))
        torch.cuda.synchronize()
    scene.stats()


KERNELS = (("pass", ("path_kernel", "list_kernel")), ("over", ("adaptive_over",)), ("count", ("adaptive_count",)),
           ("scan", ("adaptive_scan",)), ("scatter", ("adaptive_scatter",)), ("merge", ("adaptive_merge",)),
           ("reduce", ("reduce_kernel", "variance_kernel")), ("fill", ("adaptive_fill",)))


def wavefront_passes(rows, frames):
    """per listed pass of the wavefront's adaptive render: median kernel times of its generate,
    bounce-0 extend, bounce-0 shade and the rest; rows: (start, end, queue, kernel name)"""
    renders, cur = [], None
    for s, e, q, name in rows:
        if "adaptive_fill" in name:                        # the fill ends pass 0: a render's listed passes follow
            renders.append([])
            cur = None
            continue
        if not renders:
            continue
        if "wf_generate_list" in name and (cur is None or cur["merged"]):
            cur = {"generate": 0.0, "extend0": 0.0, "shade0": 0.0, "rest": 0.0, "merge": 0.0, "seen": {},
                   "t0": s, "merged": False}
            renders[-1].append(cur)
        if cur is None or cur["merged"]:
            continue
        ms = (e - s) / 1e6
        seen = cur["seen"].setdefault(q, set())
        if "wf_generate_list" in name:
            cur["generate"] += ms
            seen.clear()                                   # a new batch on this queue
        elif "adaptive_merge" in name:
            cur["merge"] += ms
            cur["wall"] = (e - cur["t0"]) / 1e6
            cur["merged"] = True
        elif "wf_extend" in name and "extend" not in seen:
            cur["extend0"] += ms
            seen.add("extend")
        elif "wf_shade_slots" in name and "shade" not in seen:
            cur["shade0"] += ms
            seen.add("shade")
        elif "wf_" in name:
            cur["rest"] += ms
    renders = [r for r in renders[1:] if r]                # the warm-up
    if len(renders) != frames:
        return {"error": f"{len(renders)} renders traced, expected {frames}"}
    out = []
    for j in range(min(len(r) for r in renders)):
        d = {"pass": j + 1}
        for k in ("generate", "extend0", "shade0", "rest", "merge", "wall"):
            v = sorted(r[j].get(k, 0.0) for r in renders)
            d[k + "_ms"] = round(v[len(v) // 2], 4)
        out.append(d)
    return {"listed_passes": out, "frames": len(renders)}


def traced_kernels(a, timeout_s=600):
    """per pass: median kernel times over the traced renders, or an error note"""
    if not shutil.which("rocprofv3"):
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="mcpt_adtrace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", "--size", str(a.size), "--spp", str(a.spp), "--chunk",
               str(a.chunk), "--passes", str(a.passes), "--trace-frames", str(a.trace_frames), "--pipeline",
               a.pipeline]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s)
        except subprocess.TimeoutExpired:
            return {"error": "traced run timed out"}
        if r.returncode != 0:
            return {"error": f"traced run failed ({r.returncode}): {r.stderr[-300:]}"}
        rows, wf_rows = [], []
        for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
            if a.keep_trace:
                os.makedirs(a.keep_trace, exist_ok=True)
                shutil.copy(f, os.path.join(a.keep_trace, os.path.basename(f)))
            with open(f) as fh:
                for row in csv.DictReader(fh):
                    name = row.get("Kernel_Name", "")
                    wf_rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row.get("Queue_Id", ""),
                                    name))
                    kind = next((k for k, pats in KERNELS if any(p in name for p in pats)), None)
                    if kind:
                        rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), kind, name))
        if a.pipeline == "wavefront":
            return wavefront_passes(sorted(wf_rows), a.trace_frames)
        rows.sort()
        # a render = from one pass-0 path kernel to the next; a pass = from one pass kernel to the next
        renders = []
        for s, e, kind, name in rows:
            if kind == "pass" and "path_kernel" in name:
                renders.append([])
            if not renders:
                continue
            if kind == "pass":
                renders[-1].append({})
            renders[-1][-1].setdefault(kind, 0.0)
            renders[-1][-1][kind] += (e - s) / 1e6
        renders = renders[1:]                              # the warm-up
        if len(renders) != a.trace_frames:
            return {"error": f"{len(renders)} renders traced, expected {a.trace_frames}"}
        npass = min(len(r) for r in renders)
        per_pass = []
        for j in range(npass):
            d = {"pass": j}
            for kind, _ in KERNELS:
                # the selection of pass j runs before its pass kernel: it sits in group j - 1
                g = j - 1 if kind in ("over", "count", "scan", "scatter") else j
                v = [r[g].get(kind, 0.0) for r in renders] if g >= 0 else []
                if any(v):
                    d[kind + "_ms"] = round(sorted(v)[len(v) // 2], 4)
            per_pass.append(d)
        total = sorted(sum(sum(p.values()) for p in r) for r in renders)[len(renders) // 2]
        return {"per_pass": per_pass, "kernels_ms": round(total, 4), "frames": len(renders)}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--pipeline", choices=["megakernel", "wavefront"], default="megakernel")
    ap.add_argument("--out", default="")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--passes", type=int, default=16)
    ap.add_argument("--trace-frames", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--keep-trace", default="", help="directory that receives the raw kernel trace csv")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    if a.trace_child:
        trace_child(a)
        return
    frame = frame_of(a)
    scene = M.Scene(M.ObjModel(M.scene_path("scene01")))
    scene.reserve(frame)
    b = Bufs(frame)
    line = {"bench": "adaptive", "device": torch.cuda.get_device_name(0), "window_s": a.window, "width": a.size,
            "height": a.size, "spp_per_pass": a.spp, "chunk": a.chunk, "passes": a.passes, "pipeline": a.pipeline}
    default = M.adaptive_params(max_passes=a.passes)
    run_adaptive = lambda: b.adaptive(scene, frame, default)   # noqa: E731
    run_uniform = lambda: b.uniform(scene, frame, a.passes)    # noqa: E731
    line["adaptive"] = with_rays(scene, timed(run_adaptive, a.window, min_reps=2), run_adaptive)
    count = b.cnt.cpu().numpy()
    line["adaptive"]["mean_passes"] = round(float(count.mean()), 4)
    active = [round(float((count > j).mean()), 5) for j in range(a.passes)]
    line["uniform"] = with_rays(scene, timed(run_uniform, a.window, min_reps=2), run_uniform)
    line["adaptive"]["ratio_to_uniform"] = round(line["adaptive"]["ms"] / line["uniform"]["ms"], 4)
    if a.pipeline == "wavefront":   # the megakernel's adaptive render of the same params, same process
        mk = dataclasses.replace(frame, pipeline="megakernel")
        scene.reserve(mk)
        run_mk = lambda: b.adaptive(scene, mk, default)        # noqa: E731
        line["megakernel_adaptive"] = timed(run_mk, a.window, min_reps=2)
        line["adaptive"]["ratio_to_megakernel_adaptive"] = round(
            line["adaptive"]["ms"] / line["megakernel_adaptive"]["ms"], 4)
    one = dataclasses.replace(frame, spp=a.spp * a.passes, spp_chunk=32)
    scene.reserve(one)
    run_one = lambda: scene.render_device(one, b.fb.data_ptr(), b.st)   # noqa: E731
    line["one_render"] = with_rays(scene, timed(run_one, a.window, min_reps=2), run_one)
    # the list's overhead: every pixel through the list against the same passes as full frames
    forced = M.adaptive_params(max_passes=4, min_passes=4, force_list=True)
    run_forced = lambda: b.adaptive(scene, frame, forced)      # noqa: E731
    run_four = lambda: b.uniform(scene, frame, 4)              # noqa: E731
    lo = {"forced_list": with_rays(scene, timed(run_forced, a.window), run_forced),
          "uniform_4": with_rays(scene, timed(run_four, a.window), run_four)}
    lo["ratio"] = round(lo["forced_list"]["ms"] / lo["uniform_4"]["ms"], 4)
    line["list_overhead"] = lo
    # per pass: rays by differencing renders cut at m passes (the counters are deterministic)
    cum = []
    for m in range(1, a.passes + 1):
        scene.stats()
        b.adaptive(scene, frame, M.adaptive_params(max_passes=m))
        torch.cuda.synchronize()
        cum.append(scene.stats()["rays"])
    rays = [cum[0]] + [cum[m] - cum[m - 1] for m in range(1, a.passes)]
    per_pass = [{"pass": j, "active": active[j], "rays": int(rays[j])} for j in range(a.passes)]
    del scene
    torch.cuda.synchronize()
    if not a.no_trace:
        tr = traced_kernels(a)
        if "error" in tr:
            line["trace_error"] = tr["error"]
        elif a.pipeline == "wavefront":
            line["listed_pass_kernels"] = tr["listed_passes"]
        else:
            for d, t in zip(per_pass, tr["per_pass"]):
                d.update({k: v for k, v in t.items() if k != "pass"})
                if d.get("pass_ms"):
                    d["Grays_per_s"] = round(d["rays"] / (d["pass_ms"] * 1e-3) / 1e9, 3)
            listed = max(1, sum(1 for d in per_pass[1:] if d["active"] > 0))
            line["adaptive"]["kernels_ms"] = tr["kernels_ms"]
            line["adaptive"]["outside_kernels_ms_per_listed_pass"] = round(
                (line["adaptive"]["ms"] - tr["kernels_ms"]) / listed, 4)
    line["per_pass"] = per_pass
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

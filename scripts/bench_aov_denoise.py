"""Times the first-hit feature buffers and the a-trous denoiser on one GPU.

    python scripts/bench_aov_denoise.py [--window 0.5] [--out profiles/aov_denoise/bench.jsonl]

Two settings, each with the frame the calls accompany, timed in the same run:
  qe   qe_scene01 read as tinyobj, 640x480, the QuinEngine viewer's 1-spp frame
  c2   scene01, 1024x1024, the C2 frame (1024 spp, wavefront pipeline, lean)
Per setting: mcpt_render_aov_device at 1 and 16 spp, mcpt_denoise_device with
its defaults (5 iterations), and the frame.  Every figure is the median of
device-event times over repeats filling a window of at least --window seconds
after a warm-up; the spread is (max - min) / median.  The denoiser's achieved
bytes/s are given against two models per pixel and iteration: 25 taps x 48 B
read + 16 B written (every tap from memory) and 64 B (each buffer once).
Prints one JSON line (and appends it to --out).
"""
import argparse
import dataclasses
import json
import os
import sys

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
    times.sort()
    med = times[len(times) // 2]
    return {"ms": round(med, 4), "spread": round((times[-1] - times[0]) / med, 4), "reps": len(times)}


def setting(name, scene, frame, window_s, iterations=5):
    W, H = frame.width, frame.height
    st = torch.cuda.current_stream().cuda_stream
    fb, ac, nd, out, scratch = (torch.zeros((H, W, 4), device="cuda") for _ in range(5))
    scene.reserve(frame)
    res = {"width": W, "height": H}
    res["frame"] = timed(lambda: scene.render_device(frame, fb.data_ptr(), st), window_s, min_reps=2)
    for spp in (1, 16):
        p = dataclasses.replace(frame, spp=spp)
        res[f"aov_spp{spp}"] = timed(lambda: scene.render_aov_device(p, ac.data_ptr(), nd.data_ptr(), st), window_s)
    gamma = frame.mode == "quinengine"
    d = timed(lambda: M.denoise_device(W, H, fb.data_ptr(), ac.data_ptr(), nd.data_ptr(), out.data_ptr(),
                                       scratch.data_ptr(), st, gamma_space=gamma), window_s)
    px_it = W * H * iterations
    d["iterations"] = iterations
    d["GBps_vs_25tap_model"] = round(px_it * (25 * 48 + 16) / (d["ms"] * 1e-3) / 1e9, 1)
    d["GBps_vs_64B_floor"] = round(px_it * 64 / (d["ms"] * 1e-3) / 1e9, 1)
    res["denoise"] = d
    for k in ("aov_spp1", "aov_spp16", "denoise"):
        res[k]["share_of_frame"] = round(res[k]["ms"] / res["frame"]["ms"], 4)
    scene.stats()
    return {name: res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default="")
    ap.add_argument("--c2-spp", type=int, default=1024)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    line = {"bench": "aov_denoise", "device": torch.cuda.get_device_name(0), "window_s": a.window}
    qe = M.Scene(M.ObjModel(M.scene_path("qe_scene01"), flavor="tinyobj"))
    line.update(setting("qe_640x480", qe, M.RenderParams.for_quinengine(seed=822569775, lean=True), a.window))
    del qe
    c2 = M.Scene(M.ObjModel(M.scene_path("scene01")))
    frame = M.RenderParams.for_scene(1, width=1024, height=1024, spp=a.c2_spp, spp_chunk=32, pipeline="wavefront",
                                     lean=True)
    line.update(setting("c2_1024x1024", c2, frame, a.window))
    line["c2_1024x1024"]["frame"]["spp"] = a.c2_spp
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

"""Times the temporal accumulation beside the stages around it on one GPU.

    python scripts/bench_temporal.py [--window 0.5] [--out profiles/temporal/bench.jsonl]

One setting: scene01 at 1024x1024, two frames of 2 spp in chunks of 1 whose cameras differ by a
2-degree yaw, 4-spp feature buffers for both.  Timed in the same run:
  mcpt_temporal_device        with and without the variance buffers
  mcpt_denoise_var_device     5 iterations, on the accumulated frame
  mcpt_render_var_device      the frame itself (megakernel, lean)
Every figure is the median of device-event times over repeats filling a window of at least
--window seconds after a warm-up; the spread is (max - min) / median.  The temporal kernel
runs for tens of microseconds, so each of its event pairs brackets --batch launches and the
time is divided by that.  Its achieved bytes/s are given against the bytes it must move --
every buffer of the call once, 16 B per pixel each: ten with the variance, seven without
(the gather's footprints overlap, so a history pixel comes from memory once).
Prints one JSON line (and appends it to --out).
"""
import argparse
import dataclasses
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import montecarlopathtracer_amd as M  # noqa: E402


def timed(fn, window_s, batch=1, min_reps=3, max_reps=2000):
    """median / spread of fn's device time per call: one warm-up, then event pairs around
    `batch` calls each for >= window_s"""
    fn()
    torch.cuda.synchronize()
    times, total = [], 0.0
    while (total < window_s * 1e3 or len(times) < min_reps) and len(times) < max_reps:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1)
        times.append(t / batch)
        total += t
    times = sorted(times)
    med = times[len(times) // 2]
    return {"ms": round(med, 5), "spread": round((times[-1] - times[0]) / med, 4), "reps": len(times), "batch": batch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    W = H = a.size
    st = torch.cuda.current_stream().cuda_stream
    scene = M.Scene(M.ObjModel(M.scene_path("scene01")))
    yaw = math.radians(2.0)
    prev = M.RenderParams.for_scene(1, width=W, height=H, spp=2, spp_chunk=1, lean=True)
    cur = dataclasses.replace(prev, direction=(math.sin(yaw), 0.0, -math.cos(yaw)), spp_offset=2)
    names = ("fb", "var", "ac", "nd", "hist", "hist_var", "hist_ac", "hist_nd", "out", "out_var", "den", "scratch")
    b = {n: torch.zeros((H, W, 4), device="cuda") for n in names}
    p = {n: t.data_ptr() for n, t in b.items()}
    scene.reserve(cur)
    # the previous frame as the history (8 frames long everywhere), then this frame
    scene.render_var_device(prev, p["hist"], p["hist_var"], st)
    scene.render_aov_device(dataclasses.replace(prev, spp=4), p["hist_ac"], p["hist_nd"], st)
    torch.cuda.synchronize()
    b["hist"][..., 3] = 8.0
    scene.render_aov_device(dataclasses.replace(cur, spp=4, spp_offset=0), p["ac"], p["nd"], st)
    line = {"bench": "temporal", "device": torch.cuda.get_device_name(0), "window_s": a.window, "width": W,
            "height": H, "spp": cur.spp, "yaw_deg": 2.0}
    line["render_var"] = timed(lambda: scene.render_var_device(cur, p["fb"], p["var"], st), a.window, min_reps=2)

    def temporal(with_var):
        v = (lambda n: p[n]) if with_var else (lambda n: 0)
        M.temporal_device(cur, prev, p["fb"], v("var"), p["ac"], p["nd"], p["hist"], v("hist_var"), p["hist_ac"],
                          p["hist_nd"], p["out"], v("out_var"), st)

    for key, with_var, nbuf in (("temporal_var", True, 10), ("temporal", False, 7)):
        t = timed(lambda: temporal(with_var), a.window, batch=a.batch)
        t["model_bytes"] = nbuf * 16 * W * H
        t["GBps_vs_model"] = round(t["model_bytes"] / (t["ms"] * 1e-3) / 1e9, 1)
        line[key] = t
    temporal(True)
    torch.cuda.synchronize()
    n = b["out"][..., 3]
    line["accumulated_share"] = round(float((n > 1).float().mean()), 4)      # pixels that found their history
    d = timed(lambda: M.denoise_var_device(W, H, p["out"], p["out_var"], p["ac"], p["nd"], p["den"], p["scratch"], st,
                                           iterations=5), a.window)
    d["iterations"] = 5
    line["denoise_var"] = d
    for key in ("temporal_var", "temporal"):
        line[key]["share_of_denoise_var"] = round(line[key]["ms"] / d["ms"], 4)
        line[key]["share_of_render_var"] = round(line[key]["ms"] / line["render_var"]["ms"], 5)
    scene.stats()
    txt = json.dumps(line)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()

"""Times the device radiance query (mcpt_radiance_device) on one GPU against the
megakernel render of the same number of paths.

    python scripts/bench_radiance.py [--window 0.5] [--out profiles/radiance/bench.jsonl]
                                     [--sizes 16,20,22] [--spp 16]

Scenes: scene01 (the image in LDS) and cornell_bunny70k (global memory, child-box cull).
Workload: the pinhole rays of the C2 camera (eye (0, 5, 17), looking down -z, 60 degrees)
through the pixel centres of a side x side frame, n = side^2 = 2^16, 2^20, 2^22 rays, --spp
samples each in one chunk, the lean kernel.
Yardstick: the lean megakernel mcpt_render_device of the side x side frame at the same spp --
the same number of paths through the same path loop, from the camera's jittered primary rays.
The two are timed alternately (query, render, query, render, ...) with device events around
each call, after a warm-up of both, until each has filled a window of at least --window
seconds; ms = the median, spread = (max - min) / median.  Rays are counted by the kernels
(lean kernels count rays only), so G rays/s is each side's own rays over its own time.
One JSON line per scene and n is printed and appended to --out.

    python scripts/bench_radiance.py --pipeline wavefront [--out profiles/radiance/bench_wf.jsonl]

times the wavefront form of the query (mcpt_radiance_ex_device, pipeline = wavefront, every
wavefront field automatic) beside the megakernel form on the same rays and parameters, the
two alternated call by call in the same way; the two outputs are compared bit for bit once
("same_bits") and ratio_time is wavefront ms / megakernel ms.
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import montecarlopathtracer_amd as M  # noqa: E402

SCENES = ["scene01", "cornell_bunny70k"]


def summary(times):
    times = sorted(times)
    med = times[len(times) // 2]
    return {"ms": round(med, 5), "spread": round((times[-1] - times[0]) / med, 4), "reps": len(times)}


def timed_alternately(fns, window_s, min_reps=3, max_reps=5000):
    """median / spread of each fn's device time: one warm-up of each, then rounds of one timed
    call of each, in turn, until every one has run for >= window_s"""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    while (min(sum(t) for t in times) < window_s * 1e3 or len(times[0]) < min_reps) and len(times[0]) < max_reps:
        for fn, t in zip(fns, times):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
    return [summary(t) for t in times]


def pixel_centre_rays(side):
    """the C2 camera's rays through the pixel centres of a side x side frame, row-major"""
    ix = torch.arange(side, device="cuda", dtype=torch.float32) + 0.5
    x = ix.repeat(side)
    y = ix.repeat_interleave(side)
    th = math.tan(math.radians(60.0) / 2)
    dx = (2 * x / side - 1) * th
    dy = (1 - 2 * y / side) * th
    d = torch.stack([dx, dy, -torch.ones_like(dx)], dim=1)
    d = (d / d.norm(dim=1, keepdim=True)).contiguous()
    o = torch.tensor([0.0, 5.0, 17.0], device="cuda").repeat(side * side, 1).contiguous()
    return o, d


def measure(scene, name, log2n, spp, window):
    n = 1 << log2n
    side = 1 << (log2n // 2)
    assert side * side == n, "n must be an even power of two"
    st = torch.cuda.current_stream().cuda_stream
    o, d = pixel_centre_rays(side)
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    fb = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    p = M.RenderParams(width=side, height=side, spp=spp, spp_chunk=spp, pipeline="megakernel", lean=True)
    scene.reserve_radiance(n, spp=spp)
    scene.reserve(p)

    def query():
        scene.radiance_device(n, o.data_ptr(), d.data_ptr(), out.data_ptr(), 0, st, spp=spp, lean=1)

    def render():
        scene.render_device(p, fb.data_ptr(), st)

    # rays of one call of each (the kernels' own counts)
    scene.trace_stats()
    query()
    torch.cuda.synchronize()
    q_rays = scene.trace_stats()["rays"]
    scene.stats()
    render()
    torch.cuda.synchronize()
    r_rays = scene.stats()["rays"]
    q, r = timed_alternately([query, render], window)
    scene.trace_stats()
    scene.stats()
    for rec, rays in ((q, q_rays), (r, r_rays)):
        rec["rays"] = int(rays)
        rec["Grays_s"] = round(rays / (rec["ms"] * 1e-3) / 1e9, 4)
        rec["Mpaths_s"] = round(n * spp / (rec["ms"] * 1e-3) / 1e6, 2)
    return {"bench": "radiance", "scene": name, "layout": "global" if scene.info()["node_boxes"] else "lds",
            "n": n, "log2n": log2n, "spp": spp, "paths": n * spp, "radiance": q, "render_megakernel": r,
            "ratio_rays_s": round(q["Grays_s"] / r["Grays_s"], 4), "ratio_paths_s": round(r["ms"] / q["ms"], 4),
            "mean_radiance": round(float(out[:, :3].mean()), 5), "mean_render": round(float(fb[:, :3].mean()), 5)}


def measure_wavefront(scene, name, log2n, spp, window):
    """the wavefront query beside the megakernel query, same rays, same parameters"""
    n = 1 << log2n
    side = 1 << (log2n // 2)
    assert side * side == n, "n must be an even power of two"
    st = torch.cuda.current_stream().cuda_stream
    o, d = pixel_centre_rays(side)
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    out_wf = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    scene.reserve_radiance(n, spp=spp)
    scene.reserve_radiance_ex(n, pipeline="wavefront", spp=spp, lean=1)

    def megakernel():
        scene.radiance_device(n, o.data_ptr(), d.data_ptr(), out.data_ptr(), 0, st, spp=spp, lean=1)

    def wavefront():
        scene.radiance_ex_device(n, o.data_ptr(), d.data_ptr(), out_wf.data_ptr(), 0, st, pipeline="wavefront", spp=spp,
                                 lean=1)

    rays = []
    for fn in (megakernel, wavefront):          # rays of one call of each (the kernels' own counts)
        scene.trace_stats()
        fn()
        torch.cuda.synchronize()
        rays.append(scene.trace_stats()["rays"])
    routes = scene.query_route_rays()
    same = bool(torch.equal(out.view(torch.int32), out_wf.view(torch.int32)))
    m, w = timed_alternately([megakernel, wavefront], window)
    scene.trace_stats()
    for rec, r in ((m, rays[0]), (w, rays[1])):
        rec["rays"] = int(r)
        rec["Grays_s"] = round(r / (rec["ms"] * 1e-3) / 1e9, 4)
        rec["Mpaths_s"] = round(n * spp / (rec["ms"] * 1e-3) / 1e6, 2)
    return {"bench": "radiance_wf", "scene": name, "layout": "global" if scene.info()["node_boxes"] else "lds",
            "n": n, "log2n": log2n, "spp": spp, "paths": n * spp, "megakernel": m, "wavefront": w,
            "ratio_time": round(w["ms"] / m["ms"], 4), "sum_spreads": round(m["spread"] + w["spread"], 4),
            "wavefront_faster_by": round(1.0 - w["ms"] / m["ms"], 4), "same_bits": same,
            "route_rays": {"direct": routes[0], "extend": routes[1], "clipped": routes[2], "sphere_skips": routes[3]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="16,20,22", help="log2 of the ray counts (even)")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--scenes", default=",".join(SCENES))
    ap.add_argument("--pipeline", default="megakernel", choices=["megakernel", "wavefront"],
                    help="wavefront: the wavefront query beside the megakernel query")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    lines = []
    for name in [s for s in a.scenes.split(",") if s]:
        scene = M.Scene(M.ObjModel(M.scene_path(name)))
        for s in [int(x) for x in a.sizes.split(",") if x]:
            if a.pipeline == "wavefront":
                # a scene per size: a wavefront reservation bounds the default batches of later,
                # larger queries (as mcpt_scene_reserve's does), and each size is to run in its own
                sized = M.Scene(M.ObjModel(M.scene_path(name)))
                lines.append(measure_wavefront(sized, name, s, a.spp, a.window))
                del sized
            else:
                lines.append(measure(scene, name, s, a.spp, a.window))
            torch.cuda.empty_cache()
        del scene
    torch.cuda.synchronize()
    dev = torch.cuda.get_device_name(0)
    for line in lines:
        line["device"] = dev
        line["window_s"] = a.window
        print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

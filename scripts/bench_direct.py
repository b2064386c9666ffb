"""Times the direct-lighting queries (mcpt_direct_device, mcpt_render_direct_device) on one GPU.

    python scripts/bench_direct.py [--window 0.5] [--out profiles/direct/bench.jsonl] [--sizes 16,20] [--spp 16]

Scenes: scene01 (the image in LDS, 12 light triangles) and cornell_bunny70k (global memory,
child-box cull).  Points: n of the closest hits of the C2 camera's pinhole rays through a
grid of 4n pixels (bench_ao.py's), their normals from the hit points' finite differences on
that grid, turned towards the camera.  Lean kernels, 16 spp.

Per scene and n, in one visit, the contenders taking turns call by call (so a drift of the
machine falls on all of them alike), each the median of device-event times over at least
--window seconds of its own calls after a warm-up; spread = (max - min) / median:
  chunk1 / chunk4 / chunk16   the fused query with spp_chunk 1, 4 and 16 (16: one chunk, no
                              partial sums and no finishing kernel)
  occluded                    mcpt_occluded_device on a pre-built buffer of the shadow rays of
                              the same construction, made with torch from the scene's light
                              table -- the light by the cdf, a uniform point on it, the same
                              bias and per-ray t_max, only the rays the fused query would walk
                              (not the same bits).  The composed path's ray generation and
                              its reduction are not in it; they are timed once (`compose_ms`,
                              `reduce_ms`).
  radiance                    mcpt_radiance_device at max_depth 1, 16 spp, along the camera rays
                              that found the points: what a caller without this query pays
                              for an estimate of the same light (a path per sample that meets
                              the lamp by chance), not the same estimator.
`ratio`: chunk1 (the fastest chunking measured) / occluded and / radiance.  `bytes`: the
device memory each needs beyond the points and normals.  The first line's `compose_ms` and
`reduce_ms` hold torch's first-call set-up.

Pixel form: frames of 2^(size/2) squared pixels x 16 spp of the C2 camera with the same three
chunkings, beside mcpt_render_aov_device at the same spp -- the primary walk alone (`aov`).
One JSON line per setting is printed and appended to --out.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import montecarlopathtracer_amd as M  # noqa: E402
from bench_rayquery import coherent, summary, unit  # noqa: E402

SCENES = ["scene01", "cornell_bunny70k"]
SEED = 20241021
BIAS = 0.01


def timed_in_turns(fns, window_s, min_reps=3, max_reps=5000):
    """{name: median / spread} of each fn's device time: one warm-up each, then the fns in
    turns, call by call, until every one has at least window_s of its own calls"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    total = {k: 0.0 for k in fns}
    while True:
        todo = [k for k in fns if (total[k] < window_s * 1e3 or len(times[k]) < min_reps) and len(times[k]) < max_reps]
        if not todo:
            break
        for k in todo:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns[k]()
            e1.record()
            e1.synchronize()
            t = e0.elapsed_time(e1)
            times[k].append(t)
            total[k] += t
    return {k: summary(v) for k, v in times.items()}


def points_of(scene, n):
    """(p, nrm, o, d) (n, 3) float32 on the device: n primary hits, their finite-difference
    normals and the camera rays that found them"""
    m = 4 * n
    side = int(round(math.sqrt(m)))
    o, d = coherent(m)
    tri = torch.empty(m, dtype=torch.int32, device="cuda")
    hit = torch.empty((m, 3), dtype=torch.float32, device="cuda")
    scene.trace_device(m, o.data_ptr(), d.data_ptr(), tri.data_ptr(), hit.data_ptr(), lean=True)
    torch.cuda.synchronize()
    P = (o + hit[:, 2:3] * d).reshape(side, side, 3)
    dx = torch.roll(P, -1, 1) - P
    dy = torch.roll(P, -1, 0) - P
    nrm = unit(torch.cross(dx, dy, dim=2).reshape(m, 3))
    nrm = torch.where((nrm * d).sum(1, keepdim=True) > 0, -nrm, nrm)
    ok = torch.nonzero((tri >= 0) & (nrm.norm(dim=1) > 0.5))[:, 0]
    assert ok.shape[0] >= n, "too few hits"
    sel = ok[torch.linspace(0, ok.shape[0] - 1, n, device="cuda").long()]
    return P.reshape(m, 3)[sel].contiguous(), nrm[sel].contiguous(), o[sel].contiguous(), d[sel].contiguous()


def light_arrays(scene, model):
    """the light table on the device: vertices (L, 3, 3), normals (L, 3), cdf (L,), the red Ka (L,),
    the total area"""
    t = scene.lights()
    tris, verts, mats = model.triangles(), model.vertices(), model.materials()
    obj = tris[scene.kd()[2][t["kd_ids"]]]           # kd id -> OBJ triangle
    v = verts[obj[:, :3]].astype(np.float32)
    ka = mats[obj[:, 9], 0].astype(np.float32)
    return (torch.from_numpy(v).cuda(), torch.from_numpy(t["normals"]).cuda(), torch.from_numpy(t["cdf"]).cuda(),
            torch.from_numpy(ka).cuda(), float(t["area_total"]))


def compose(p, nrm, lights, spp, gen):
    """the composed path's shadow rays, point-major: (o, d, t_max) of the rays the fused query
    would walk, their owner (point index), and what each adds to its point's red channel if
    unoccluded (illum 10)"""
    lv, ln, cdf, ka, area = lights
    n = p.shape[0]
    u = torch.rand((3, n, spp), device="cuda", generator=gen)
    j = torch.searchsorted(cdf, u[0].contiguous(), right=True).clamp_max(cdf.shape[0] - 1)
    su = u[1].sqrt()
    b, c = (su * (1 - u[2]))[..., None], (su * u[2])[..., None]
    y = lv[j, 0] * (1 - b - c) + lv[j, 1] * b + lv[j, 2] * c
    w = y - p[:, None]
    r2 = (w * w).sum(-1)
    r = r2.sqrt()
    d = w / r[..., None]
    cx = (nrm[:, None] * d).sum(-1)
    cy = (ln[j] * d).sum(-1).abs()
    ok = (cx > 0) & (cy > 0) & (r > 2 * BIAS)
    g = cx * cy * area / (math.pi * r2) * ka[j] * 10.0
    o = p[:, None] + BIAS * d
    owner = torch.arange(n, device="cuda")[:, None].expand(n, spp)
    return (o[ok].contiguous(), d[ok].contiguous(), (r - 2 * BIAS)[ok].contiguous(), owner[ok].contiguous(),
            g[ok].contiguous())


def point_lines(scene, lights, name, n, spp, window):
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(SEED + n)
    p, nrm, ro, rd = points_of(scene, n)
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    rad = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    o, d, tm, owner, g = compose(p, nrm, lights, spp, gen)
    m = o.shape[0]
    occ = torch.empty(m, dtype=torch.uint8, device="cuda")
    e1.record()
    e1.synchronize()
    compose_ms = e0.elapsed_time(e1)
    fns = {f"chunk{c}": (lambda c=c: scene.direct_device(n, p.data_ptr(), nrm.data_ptr(), out.data_ptr(), 0, st, spp=spp,
                                                         spp_chunk=c, lean=True)) for c in (1, 4, spp)}
    fns["occluded"] = lambda: scene.occluded_device(m, o.data_ptr(), d.data_ptr(), occ.data_ptr(), tm.data_ptr(), st,
                                                    lean=True)
    fns["radiance"] = lambda: scene.radiance_device(n, ro.data_ptr(), rd.data_ptr(), rad.data_ptr(), 0, st, spp=spp,
                                                    max_depth=1, lean=True)
    line = {"bench": "direct_points", "scene": name, "n": n, "log2n": int(math.log2(n)), "spp": spp,
            "samples": n * spp, "shadow_rays": m}
    line.update(timed_in_turns(fns, window))
    scene.trace_stats()
    scene.direct_device(n, p.data_ptr(), nrm.data_ptr(), out.data_ptr(), 0, st, spp=spp, spp_chunk=spp, lean=True)
    torch.cuda.synchronize()
    line["fused_shadow_rays"] = int(scene.trace_stats()["rays"])
    e0.record()
    red = torch.zeros(n, device="cuda").index_add_(0, owner, g * (occ == 0).float()) / spp
    e1.record()
    e1.synchronize()
    line["ratio"] = {k: round(line["chunk1"]["ms"] / line[k]["ms"], 4) for k in ("occluded", "radiance")}
    line["compose_ms"] = round(compose_ms, 4)
    line["reduce_ms"] = round(e0.elapsed_time(e1), 4)
    # the mean red channel over the points: the two constructions agree statistically
    line["mean_red"] = {"fused": round(float(out[:, 0].mean()), 5), "composed": round(float(red.mean()), 5)}
    line["bytes"] = {"fused_chunk16": 0, "fused_chunk1": n * spp * 16, "composed": m * 29 + n * spp * 8}
    return [line]


def frame_lines(scene, name, size, spp, window):
    st = torch.cuda.current_stream().cuda_stream
    rp = M.RenderParams(width=size, height=size, spp=spp, lean=True)
    out = torch.empty(size * size * 4, dtype=torch.float32, device="cuda")
    ac = torch.empty(size * size * 4, dtype=torch.float32, device="cuda")
    nd = torch.empty(size * size * 4, dtype=torch.float32, device="cuda")
    fns = {f"chunk{c}": (lambda c=c: scene.render_direct_device(rp, out.data_ptr(), st, spp_chunk=c, lean=True))
           for c in (1, 4, spp)}
    fns["aov"] = lambda: scene.render_aov_device(rp, ac.data_ptr(), nd.data_ptr(), st)
    line = {"bench": "direct_frame", "scene": name, "width": size, "height": size, "spp": spp}
    line.update(timed_in_turns(fns, window))
    line["ratio"] = {"aov": round(line["chunk1"]["ms"] / line["aov"]["ms"], 4)}
    scene.trace_stats()
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="16,20", help="log2 of the point and pixel counts (even)")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--scenes", default=",".join(SCENES))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    lines = []
    for name in a.scenes.split(","):
        model = M.ObjModel(M.scene_path(name))
        scene = M.Scene(model)
        lights = light_arrays(scene, model)
        sizes = [int(x) for x in a.sizes.split(",") if x]
        scene.reserve_direct(max(1 << s for s in sizes), spp=a.spp, spp_chunk=1)
        for s in sizes:
            lines += point_lines(scene, lights, name, 1 << s, a.spp, a.window)
            torch.cuda.empty_cache()
            lines += frame_lines(scene, name, 1 << (s // 2), a.spp, a.window)
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

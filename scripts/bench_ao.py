"""Times the ambient-occlusion queries (mcpt_ao_device, mcpt_render_ao_device) on one GPU.

    python scripts/bench_ao.py [--window 0.5] [--out profiles/ao/bench.jsonl] [--sizes 16,18,20] [--spp 16]

Scenes: scene01 (the image in LDS) and cornell_bunny70k (global memory, child-box cull).
Points: n of the closest hits of the C2 camera's pinhole rays through a grid of 4n pixels
(spread evenly over the hits), their normals from the hit points' finite differences on
that grid, turned towards the camera.  Lean kernels, 16 spp, radius unbounded and 2.

Per scene, n and radius: the fused query (`fused`), and beside it the yardstick of the same
visit -- mcpt_occluded_device on a buffer of n x spp rays of the same construction, built
with torch: cosine-hemisphere directions about the same normals from the same points, the
same bias and t_max (`occluded`; not the same bits).  Each is the median of device-event
times over repeats filling a window of at least --window seconds after a warm-up; spread =
(max - min) / median.  `ratio` = fused / occluded: the yardstick leaves the composed path's
ray generation and flag reduction uncounted (timed once as `compose_ms`), so a ratio up to 1
plus the spreads means the fused form wins end to end.  `bytes`: the device memory each
needs beyond the n points and normals (fused: one count and one float per point; composed:
the rays and the flags).  `units`: the fused query with explicit samples per work unit.

Pixel form: 1024^2 x 16 spp of the C2 frame (`frame`), beside mcpt_render_aov_device at the
same spp -- the primary walk alone (`aov`).  One JSON line per setting is printed and appended
to --out.
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import montecarlopathtracer_amd as M  # noqa: E402
from bench_rayquery import coherent, timed, unit  # noqa: E402

SCENES = ["scene01", "cornell_bunny70k"]
SEED = 20241021
BIAS = 0.01


def points_of(scene, n):
    """(p, nrm) (n, 3) float32 on the device: n primary hits and their finite-difference normals"""
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
    return P.reshape(m, 3)[sel].contiguous(), nrm[sel].contiguous()


def compose(p, nrm, spp, gen):
    """the composed path's ray buffer: (o, d) (n * spp, 3), point-major"""
    n = p.shape[0]
    u1 = torch.rand((n, spp), device="cuda", generator=gen)
    u2 = torch.rand((n, spp), device="cuda", generator=gen)
    r, phi = u1.sqrt(), 2 * math.pi * u2
    a = torch.where(nrm[:, 1:2].abs() < 0.9, torch.tensor([0.0, 1.0, 0.0], device="cuda"),
                    torch.tensor([1.0, 0.0, 0.0], device="cuda"))
    t = unit(torch.cross(a.expand_as(nrm), nrm, dim=1))
    b = torch.cross(nrm, t, dim=1)
    d = ((r * phi.cos())[..., None] * t[:, None] + (1 - u1).sqrt()[..., None] * nrm[:, None] +
         (r * phi.sin())[..., None] * b[:, None])
    o = p[:, None] + BIAS * d
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


def point_lines(scene, name, n, spp, window, sweep):
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(SEED + n)
    p, nrm = points_of(scene, n)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    o, d = compose(p, nrm, spp, gen)
    occ = torch.empty(n * spp, dtype=torch.uint8, device="cuda")
    e1.record()
    e1.synchronize()
    compose_ms = e0.elapsed_time(e1)
    lines = []
    for radius in (0.0, 2.0):
        def fused(**kw):
            return timed(lambda: scene.ao_device(n, p.data_ptr(), nrm.data_ptr(), out.data_ptr(), 0, st, spp=spp,
                                                 radius=radius, lean=True, **kw), window)
        line = {"bench": "ao_points", "scene": name, "n": n, "log2n": int(math.log2(n)), "spp": spp,
                "radius": radius, "rays": n * spp}
        line["fused"] = fused()
        open_share = float(out.mean())
        line["occluded"] = timed(lambda: scene.occluded_device(n * spp, o.data_ptr(), d.data_ptr(), occ.data_ptr(), 0,
                                                               st, t_max=radius, lean=True), window)
        e0.record()
        red = 1.0 - occ.reshape(n, spp).float().mean(1)
        e1.record()
        e1.synchronize()
        line["ratio"] = round(line["fused"]["ms"] / line["occluded"]["ms"], 4)
        line["Grays_s"] = {k: round(n * spp / (line[k]["ms"] * 1e-3) / 1e9, 4) for k in ("fused", "occluded")}
        line["compose_ms"] = round(compose_ms, 4)
        line["reduce_ms"] = round(e0.elapsed_time(e1), 4)
        line["open_share"] = {"fused": round(open_share, 4), "occluded": round(float(red.mean()), 4)}
        line["bytes"] = {"fused": n * 8, "composed": n * spp * 25 + n * 4}
        if sweep:
            line["units"] = {str(u): fused(unit_samples=u) for u in (1, 4, spp)}
        lines.append(line)
    scene.trace_stats()
    return lines


def frame_lines(scene, name, size, spp, window):
    st = torch.cuda.current_stream().cuda_stream
    rp = M.RenderParams(width=size, height=size, spp=spp, lean=True)
    out = torch.empty(size * size, dtype=torch.float32, device="cuda")
    ac = torch.empty(size * size * 4, dtype=torch.float32, device="cuda")
    nd = torch.empty(size * size * 4, dtype=torch.float32, device="cuda")
    line = {"bench": "ao_frame", "scene": name, "width": size, "height": size, "spp": spp}
    line["aov"] = timed(lambda: scene.render_aov_device(rp, ac.data_ptr(), nd.data_ptr(), st), window)
    for radius in (0.0, 2.0):
        line[f"frame_r{radius:g}"] = timed(lambda: scene.render_ao_device(rp, out.data_ptr(), st, radius=radius,
                                                                          lean=True), window)
        line[f"open_share_r{radius:g}"] = round(float(out.mean()), 4)
    scene.trace_stats()
    return [line]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="16,18,20", help="log2 of the point counts (even)")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--frame", type=int, default=1024, help="side of the pixel form's frame (0: skip)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    lines = []
    for name in SCENES:
        scene = M.Scene(M.ObjModel(M.scene_path(name)))
        sizes = [int(x) for x in a.sizes.split(",") if x]
        scene.reserve_ao(max([1 << s for s in sizes] + [a.frame * a.frame]))
        for s in sizes:
            lines += point_lines(scene, name, 1 << s, a.spp, a.window, sweep=s in (16, 20))
            torch.cuda.empty_cache()
        if a.frame:
            lines += frame_lines(scene, name, a.frame, a.spp, a.window)
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

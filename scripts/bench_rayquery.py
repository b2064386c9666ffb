"""Times the device ray queries (mcpt_trace_device, mcpt_occluded_device) on one GPU.

    python scripts/bench_rayquery.py [--window 0.5] [--out profiles/rayquery/bench.jsonl]
                                     [--sizes 10,16,20,24] [--baseline-sizes 20,22] [--keep-trace DIR]

Scenes: scene01 (the image in LDS) and cornell_bunny70k (global memory, child-box cull).
Three ray sets, built with torch on the device from a fixed seed:
  coherent    pinhole rays of the C2 camera through a 4096^2 grid (a strided subset for n < 2^24)
  incoherent  origins at the coherent set's hit points, pulled back 0.01 along the ray, with
              uniformly random unit directions
  shadow      the same origins aimed at random points of the emitting triangles (the ceiling
              light), t_max = 0.999 x the distance; through both entries
Per scene, set and n: G rays/s of trace_device and occluded_device (lean kernels; the counting
closest-hit kernel too), each the median of device-event times over repeats filling a window
of at least --window seconds after a warm-up; spread = (max - min) / median.  One JSON line
per setting is printed and appended to --out.

Threshold rows (n = 2^10, 2^16, coherent set): the same query with an explicit number of
workgroups, i.e. rays per workgroup -- the candidates for the automatic grid's floor.

Baseline: the kernel time of mcpt_intersect's query_kernel on the same rays (t_max = FLT_MAX;
trace_device is timed without a limit beside it), from a child process run under
`rocprofv3 --kernel-trace` -- a run of its own, no counters.
"""
import argparse
import csv
import glob
import json
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import montecarlopathtracer_amd as M  # noqa: E402

SCENES = ["scene01", "cornell_bunny70k"]
SETS = ["coherent", "incoherent", "shadow"]
SEED = 20240923


def summary(times):
    times = sorted(times)
    med = times[len(times) // 2]
    return {"ms": round(med, 5), "spread": round((times[-1] - times[0]) / med, 4), "reps": len(times)}


def timed(fn, window_s, min_reps=3, max_reps=5000):
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


def light_triangles(model):
    """(m, 3, 3) float32 vertices of the triangles whose material emits (Ka > 0)"""
    tris, mats, verts = model.triangles(), model.materials(), model.vertices()
    emit = (mats[:, :3] > 0).any(axis=1)
    sel = tris[emit[tris[:, 9]]]
    assert sel.shape[0] > 0, "the scene has no emitter"
    return verts[sel[:, :3]].astype(np.float32)


def unit(v):
    return v / v.norm(dim=1, keepdim=True).clamp_min(1e-30)


def coherent(n):
    """pinhole rays of the C2 camera (eye (0, 5, 17), looking down -z, 60 degrees) through the
    centres of a strided subset of a 4096^2 pixel grid"""
    side = int(round(math.sqrt(n)))
    assert side * side == n, "n must be an even power of two"
    step = 4096 // side
    ix = (torch.arange(side, device="cuda", dtype=torch.float32) * step + 0.5 * step)
    x = ix.repeat(side)
    y = ix.repeat_interleave(side)
    th = math.tan(math.radians(60.0) / 2)
    dx = (2 * x / 4096 - 1) * th
    dy = (1 - 2 * y / 4096) * th
    d = unit(torch.stack([dx, dy, -torch.ones_like(dx)], dim=1)).contiguous()
    o = torch.tensor([0.0, 5.0, 17.0], device="cuda").repeat(n, 1).contiguous()
    return o, d


def ray_sets(scene, lights, n):
    """{set: (o, d, t_max or None)} on the device"""
    g = torch.Generator(device="cuda")
    g.manual_seed(SEED + n)
    o, d = coherent(n)
    tri = torch.empty(n, dtype=torch.int32, device="cuda")
    hit = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    scene.trace_device(n, o.data_ptr(), d.data_ptr(), tri.data_ptr(), hit.data_ptr(), lean=True)
    torch.cuda.synchronize()
    t = torch.where(tri >= 0, hit[:, 2] - 0.01, torch.zeros_like(hit[:, 2]))
    o2 = (o + t[:, None] * d).contiguous()
    d2 = unit(torch.randn((n, 3), device="cuda", generator=g)).contiguous()
    lt = torch.from_numpy(lights).cuda()
    k = torch.randint(0, lt.shape[0], (n,), device="cuda", generator=g)
    a, b = torch.rand(n, device="cuda", generator=g), torch.rand(n, device="cuda", generator=g)
    sw = a + b > 1
    a, b = torch.where(sw, 1 - a, a), torch.where(sw, 1 - b, b)
    v = lt[k]
    p = v[:, 0] + a[:, None] * (v[:, 1] - v[:, 0]) + b[:, None] * (v[:, 2] - v[:, 0])
    to = p - o2
    dist = to.norm(dim=1)
    d3 = unit(to).contiguous()
    tm = (0.999 * dist).contiguous()
    return {"coherent": (o, d, None), "incoherent": (o2, d2, None), "shadow": (o2, d3, tm)}


def measure(scene, name, sets, n, window):
    lines = []
    st = torch.cuda.current_stream().cuda_stream
    tri = torch.empty(n, dtype=torch.int32, device="cuda")
    hit = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    occ = torch.empty(n, dtype=torch.uint8, device="cuda")
    for sname in SETS:
        o, d, tm = sets[sname]
        tp = tm.data_ptr() if tm is not None else 0

        def rate(r):
            r["Grays_s"] = round(n / (r["ms"] * 1e-3) / 1e9, 4)
            return r
        line = {"bench": "rayquery", "scene": name, "set": sname, "n": n, "log2n": int(math.log2(n))}
        line["trace"] = rate(timed(lambda: scene.trace_device(n, o.data_ptr(), d.data_ptr(), tri.data_ptr(),
                                                              hit.data_ptr(), tp, st, lean=True), window))
        line["trace_counting"] = rate(timed(lambda: scene.trace_device(n, o.data_ptr(), d.data_ptr(), tri.data_ptr(),
                                                                       hit.data_ptr(), tp, st), window))
        line["occluded"] = rate(timed(lambda: scene.occluded_device(n, o.data_ptr(), d.data_ptr(), occ.data_ptr(),
                                                                    tp, st, lean=True), window))
        if tm is not None:    # beside the baseline, which has no per-ray limit
            line["trace_counting_no_limit"] = rate(timed(
                lambda: scene.trace_device(n, o.data_ptr(), d.data_ptr(), tri.data_ptr(), hit.data_ptr(), 0, st),
                window))
        line["hit_fraction"] = round(float((tri >= 0).float().mean()), 4)
        line["occluded_fraction"] = round(float((occ != 0).float().mean()), 4)
        lines.append(line)
    scene.trace_stats()
    return lines


def threshold_rows(scene, name, sets, n, window, in_lds):
    """the coherent set with explicit workgroup counts: rays per workgroup against time"""
    o, d, _ = sets["coherent"]
    st = torch.cuda.current_stream().cuda_stream
    tri = torch.empty(n, dtype=torch.int32, device="cuda")
    hit = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    full = 256 if in_lds else 1024
    rows = {}
    for per in (64, 128, 256, 512, 1024, 2048, 4096):
        wg = -(-n // per)
        if wg > full or wg < 1:
            continue
        r = timed(lambda: scene.trace_device(n, o.data_ptr(), d.data_ptr(), tri.data_ptr(), hit.data_ptr(), 0, st,
                                             lean=True, workgroups=wg), window / 4)
        rows[str(per)] = {"workgroups": wg, **r}
    auto = timed(lambda: scene.trace_device(n, o.data_ptr(), d.data_ptr(), tri.data_ptr(), hit.data_ptr(), 0, st,
                                            lean=True), window / 4)
    return {"bench": "rayquery_threshold", "scene": name, "n": n, "rays_per_workgroup": rows, "automatic": auto}


def baseline_child(sizes):
    """mcpt_intersect on the three sets, three calls each (the first is the warm-up)"""
    for name in SCENES:
        model = M.ObjModel(M.scene_path(name))
        scene = M.Scene(model)
        lights = light_triangles(model)
        for n in sizes:
            sets = ray_sets(scene, lights, n)
            for sname in SETS:
                o, d, _ = sets[sname]
                oh, dh = o.cpu().numpy(), d.cpu().numpy()
                for _ in range(3):
                    scene.intersect(oh, dh)
        del scene


def baseline(sizes, keep, timeout_s=900):
    """{scene: {set: {n: query_kernel ms}}} from a kernel trace of a child process, or an error note"""
    if not shutil.which("rocprofv3"):
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="mcpt_rqtrace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "run", "--", sys.executable,
               os.path.abspath(__file__), "--baseline-child", "--baseline-sizes", ",".join(str(s) for s in sizes)]
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
                    if "query_kernel" in row.get("Kernel_Name", ""):
                        rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
        rows.sort()
        want = len(SCENES) * len(sizes) * len(SETS) * 3
        if len(rows) != want:
            return {"error": f"{len(rows)} query_kernel dispatches traced, expected {want}"}
        res, i = {}, 0
        for name in SCENES:
            for n in [1 << s for s in sizes]:
                for sname in SETS:
                    mine = [(e - s) / 1e6 for s, e in rows[i + 1:i + 3]]
                    i += 3
                    res.setdefault(name, {}).setdefault(sname, {})[str(n)] = {
                        "ms": round(min(mine), 5), "ms_other": round(max(mine), 5),
                        "Grays_s": round(n / (min(mine) * 1e-3) / 1e9, 4)}
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", default="10,16,20,24", help="log2 of the ray counts (even)")
    ap.add_argument("--baseline-sizes", default="20,22")
    ap.add_argument("--baseline-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--keep-trace", default="", help="directory that receives the raw kernel trace csv")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    bsizes = [int(s) for s in a.baseline_sizes.split(",") if s]
    if a.baseline_child:
        baseline_child([1 << s for s in bsizes])
        return
    lines = []
    for name in SCENES:
        model = M.ObjModel(M.scene_path(name))
        scene = M.Scene(model)
        in_lds = not scene.info()["node_boxes"]
        lights = light_triangles(model)
        scene.reserve_rays()
        for s in [int(x) for x in a.sizes.split(",") if x]:
            n = 1 << s
            sets = ray_sets(scene, lights, n)
            lines += measure(scene, name, sets, n, a.window)
            if s in (10, 16):
                lines.append(threshold_rows(scene, name, sets, n, a.window, in_lds))
            del sets
            torch.cuda.empty_cache()
        del scene
    torch.cuda.synchronize()
    if not a.no_baseline:
        lines.append({"bench": "rayquery_baseline", "kernel": "query_kernel (mcpt_intersect)",
                      "source": "rocprofv3 --kernel-trace, child process", **baseline(bsizes, a.keep_trace)})
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

"""Price the clip walk (render_launch.hpp "Clip walk") on the CPU oracle's own
path loop (no GPU): of a render's secondary rays, how many the miss cull takes
(no occluder box hit), the direct resolve (one box, a listed one) and the walk;
of the walked rays, how many carry a selector (at least one box without a list,
at most one with a list), their share of all secondary inner visits and triangle
tests, their box patterns by share of inner visits, and what the clipped walk --
the same ordered walk from the root with the interval cut to the union of the
selector's unlisted boxes' slab intervals -- spends instead: inner visits, tests,
the steps of its single-child prefix, how many find a hit, and how many hit ids
differ from the full walk's (must be 0, with and without the listed box's
triangles on top).  The boxes and lists are the product's (Scene.miss_cull_boxes,
Scene.direct_lists).  See scripts/price_clip_walk.c.  Diagnostic only.

  python scripts/price_clip_walk.py [scene01] [size] [spp]
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
SO = "/tmp/mcpt_price_clip_walk.so"
NAMES = ["secondary", "nobox", "direct", "walked", "walk_inner", "walk_tests", "sel", "sel_inner", "sel_tests",
         "clip_inner", "clip_tests", "clip_prefix", "clip_hits", "clip_hit_diff", "final_diff", "empty"]


def build():
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO,
                    os.path.join(ROOT, "scripts", "price_clip_walk.c"), os.path.join(ROOT, "oracle", "obj_reader.c"),
                    os.path.join(ROOT, "oracle", "kdtree_ref.c"), "-I", os.path.join(ROOT, "oracle"), "-lm",
                    "-pthread"], check=True)


def main():
    scene = sys.argv[1] if len(sys.argv) > 1 else "scene01"
    size = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    spp = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    build()
    import oracle
    oracle.LIB_PATH = SO
    L = oracle.lib()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.diag_init.argtypes = [C.POINTER(C.c_float), C.c_int, ip, ip, C.c_int]
    L.diag_read.argtypes = [dp, dp]
    assert L.diag_nacc() == len(NAMES)
    import montecarlopathtracer_amd as M
    path = M.scene_path(scene)
    ps = M.Scene(M.ObjModel(path), host_only=True)
    boxes = np.ascontiguousarray(ps.miss_cull_boxes())
    dl = ps.direct_lists()
    print(f"{scene}: {len(boxes)} occluder boxes, triangles per box {dl['box_tris'].tolist()}, "
          f"listed boxes {np.flatnonzero(dl['counts']).tolist()}")
    if not len(boxes) or not dl["counts"].any():
        print("  no boxes or no lists: no selectors")
        return
    counts = np.zeros(8, np.int32)
    counts[: len(boxes)] = dl["counts"]
    lists = np.full((8, 16), -1, np.int32)
    lists[: len(boxes), : dl["list_kd"].shape[1]] = dl["list_kd"]
    L.diag_init(boxes.ctypes.data_as(C.POINTER(C.c_float)), len(boxes), counts.ctypes.data_as(ip),
                np.ascontiguousarray(lists).ctypes.data_as(ip), 16)
    s = oracle.Scene(path)
    # the whole C2 view at size x size; one thread: the hooks' sums are global
    _, c = s.render(oracle.RenderParams(width=size, height=size, spp=spp, spp_chunk=spp, traversal=oracle.KD_ORDERED,
                                        threads=1))
    acc = (C.c_double * len(NAMES))()
    pat = (C.c_double * (256 * 3))()
    L.diag_read(acc, pat)
    a = dict(zip(NAMES, acc[:]))
    p = np.array(pat[:]).reshape(256, 3)
    n = lambda k: int(a[k])  # noqa: E731
    sel = max(a["sel"], 1)
    # every secondary ray's walk: the oracle's counters minus the primary rays' are not split, so the
    # shares below are of the rays that hit a box (the culled ones' walks are no extend's work)
    print(f"  {size}x{size} x {spp} spp: rays {c['rays']}, secondary {n('secondary')}: {n('nobox')} hit no box (miss cull), "
          f"{n('direct')} one listed box (direct resolve), {n('walked')} walked")
    print(f"  selected {n('sel')}: {a['sel'] / max(a['walked'], 1):.1%} of the walked, {a['sel'] / max(a['secondary'], 1):.1%} of "
          f"all secondary, {a['sel'] / max(a['secondary'] - a['nobox'], 1):.1%} of those that hit a box")
    print(f"    full walk: {a['sel_inner'] / sel:.1f} inner visits, {a['sel_tests'] / sel:.1f} tests per ray "
          f"(walked rays: {a['walk_inner'] / max(a['walked'], 1):.1f} / {a['walk_tests'] / max(a['walked'], 1):.1f}); "
          f"{a['sel_inner'] / max(a['walk_inner'], 1):.1%} of the walked rays' inner visits, "
          f"{a['sel_tests'] / max(a['walk_tests'], 1):.1%} of their tests")
    print(f"    clipped walk: {a['clip_inner'] / sel:.1f} inner visits ({a['clip_inner'] / max(a['sel_inner'], 1) - 1:+.0%}), "
          f"{a['clip_tests'] / sel:.1f} tests ({a['clip_tests'] / max(a['sel_tests'], 1) - 1:+.0%}), "
          f"{a['clip_prefix'] / sel:.1f} steps of single-child prefix, {n('empty')} empty intervals")
    print(f"    {a['clip_hits'] / sel:.1%} of the clipped walks find a hit ({n('clip_hits')}), {n('clip_hit_diff')} with another "
          f"hit id than the walk's; with the listed box's triangles on top {n('final_diff')} of {n('sel')} differ")
    # a start below the root (the issue's second step), priced statically: per unlisted box, the depth of
    # the deepest KD node whose cell (by the split planes) holds the box grown by 2^-12 of the scene's
    # extent -- the inner steps a ray whose selector names that box alone would skip
    nodes = s.kd_nodes()
    ext = float((boxes[:, 3:].max(axis=0) - boxes[:, :3].min(axis=0)).max()) * 2.0 ** -12
    saved = 0.0
    for b in np.flatnonzero(dl["counts"] == 0):
        node, depth = 0, 0
        while nodes[node, 2]:
            ax = int(nodes[node, 2]) - 1
            sv = float(nodes[node, 3:4].view(np.float32)[0])
            if boxes[b, 3 + ax] + ext < sv:
                node = int(nodes[node, 0])
            elif boxes[b, ax] - ext > sv:
                node = int(nodes[node, 1])
            else:
                break
            depth += 1
        only = sum(p[m, 0] for m in range(256) if (m & ~sum(1 << int(i) for i in np.flatnonzero(dl["counts"]))) == 1 << b)
        saved += depth * only
        print(f"    start below the root, box {b}: its cell's node is at depth {depth}; {int(only)} selected rays name it alone")
    print(f"    static saving of a start below the root: {saved / sel:.2f} inner steps per selected ray")
    order = np.argsort(-p[:, 1])
    print("    patterns by share of the selected rays' inner visits:")
    for m in order[:8]:
        if p[m, 0]:
            bx = [b for b in range(8) if (m >> b) & 1]
            print(f"      {bx}: {int(p[m, 0])} rays, {p[m, 1] / max(a['sel_inner'], 1):.1%} of inner visits "
                  f"({p[m, 1] / max(a['walk_inner'], 1):.1%} of the walked rays'), {p[m, 1] / p[m, 0]:.1f} / {p[m, 2] / p[m, 0]:.1f} per ray")


if __name__ == "__main__":
    main()

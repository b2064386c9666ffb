"""Price the miss cull (render_launch.hpp "Miss cull") on the CPU oracle's own
path loop (no GPU): per bounce, the share of secondary rays that miss, that
fail every occluder box of the scene (the product's boxes, the product's slab
test), whether any box-failing ray had a hit (must be 0), and the walk's cost
of the rays the cull would take (see scripts/price_miss_cull.c).  Diagnostic only.

  python scripts/price_miss_cull.py [scene01] [size] [spp]
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
SO = "/tmp/mcpt_price_miss_cull.so"


def build():
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO,
                    os.path.join(ROOT, "scripts", "price_miss_cull.c"), os.path.join(ROOT, "oracle", "obj_reader.c"),
                    os.path.join(ROOT, "oracle", "kdtree_ref.c"), "-I", os.path.join(ROOT, "oracle"), "-lm",
                    "-pthread"], check=True)


def main():
    scene = sys.argv[1] if len(sys.argv) > 1 else "scene01"
    size = int(sys.argv[2]) if len(sys.argv) > 2 else 160
    spp = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    build()
    import oracle
    oracle.LIB_PATH = SO
    L = oracle.lib()
    L.diag_init.argtypes = [C.POINTER(C.c_float), C.c_int]
    L.diag_read.argtypes = [C.POINTER(C.c_double)]
    import montecarlopathtracer_amd as M
    path = M.scene_path(scene)
    boxes = np.ascontiguousarray(M.Scene(M.ObjModel(path), host_only=True).miss_cull_boxes())
    print(f"{scene}: {len(boxes)} occluder boxes")
    if not len(boxes):
        return
    L.diag_init(boxes.ctypes.data_as(C.POINTER(C.c_float)), len(boxes))
    s = oracle.Scene(path)
    # the whole C2 view at size x size (every region sampled); one thread: the hooks' sums are global
    _, c = s.render(oracle.RenderParams(width=size, height=size, spp=spp, spp_chunk=spp, traversal=oracle.KD_ORDERED,
                                        threads=1))
    acc = (C.c_double * (16 * 8))()
    L.diag_read(acc)
    a = np.array(acc[:]).reshape(16, 8)
    print(f"  {size}x{size} x {spp} spp: rays {c['rays']}, secondary {int(a[:, 0].sum())}; all rays: inner "
          f"{c['inner_visits'] / c['rays']:.1f} tests {c['tri_tests'] / c['rays']:.1f} per ray")
    print("  depth     rays   miss  fail-all-boxes  of-those-hit  inner/tests all   inner/tests box-failing")
    for dpt in range(1, 16):
        n, miss, fail, bad, i_all, t_all, i_f, t_f = a[dpt]
        if not n:
            continue
        print(f"  {dpt:5d} {int(n):8d} {miss / n:6.1%} {fail / n:15.1%} {int(bad):13d}  {i_all / n:8.1f} /{t_all / n:5.1f}"
              f"   {i_f / max(fail, 1):10.1f} /{t_f / max(fail, 1):5.1f}")
    n, miss, fail, bad, i_all, t_all, i_f, t_f = a.sum(axis=0)
    print(f"  secondary rays: {fail / n:.1%} culled = {fail / max(miss, 1):.1%} of the misses, {int(bad)} of them had a hit; "
          f"they hold {i_f / i_all:.1%} of the secondary inner visits and {t_f / t_all:.1%} of the triangle tests")


if __name__ == "__main__":
    main()

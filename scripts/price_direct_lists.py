"""Price the direct lists (render_launch.hpp "Direct lists") on the CPU oracle's
own path loop (no GPU): per bounce, the share of the walked secondary rays (those
that hit at least one occluder box: the miss cull takes the others) that are
direct -- exactly one box hit, and a listed one -- their share of the walk's
inner visits and triangle tests, and how many direct rays' list result differs
from the ordered walk's hit id (must be 0).  The boxes and the assignment of
triangles to them are the product's (Scene.miss_cull_boxes, Scene.direct_lists);
K = 0 prices the product's own lists, another K the lists that K would give.
See scripts/price_direct_lists.c.  Diagnostic only.

  python scripts/price_direct_lists.py [scene01] [size] [spp] [K,K,...]
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
SO = "/tmp/mcpt_price_direct_lists.so"


def build():
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-ffp-contract=off", "-shared", "-fPIC", "-o", SO,
                    os.path.join(ROOT, "scripts", "price_direct_lists.c"), os.path.join(ROOT, "oracle", "obj_reader.c"),
                    os.path.join(ROOT, "oracle", "kdtree_ref.c"), "-I", os.path.join(ROOT, "oracle"), "-lm",
                    "-pthread"], check=True)


def lists_for(dl, k):
    """(counts, lists (boxes, 16) kd ids) that K = k gives from the product's assignment"""
    n = len(dl["box_tris"])
    counts = np.zeros(16, np.int32)
    lists = np.full((16, 16), -1, np.int32)
    for b in range(n):
        ids = np.flatnonzero(dl["tri_box"] == b)
        if 1 <= len(ids) <= k:
            counts[b] = len(ids)
            lists[b, : len(ids)] = ids
    return counts, lists


def main():
    scene = sys.argv[1] if len(sys.argv) > 1 else "scene01"
    size = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    spp = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    ks = [int(x) for x in sys.argv[4].split(",")] if len(sys.argv) > 4 else [0]
    build()
    import oracle
    oracle.LIB_PATH = SO
    L = oracle.lib()
    ip = C.POINTER(C.c_int)
    L.diag_init.argtypes = [C.POINTER(C.c_float), C.c_int, ip, ip, C.c_int]
    L.diag_read.argtypes = [C.POINTER(C.c_double)]
    import montecarlopathtracer_amd as M
    path = M.scene_path(scene)
    ps = M.Scene(M.ObjModel(path), host_only=True)
    boxes = np.ascontiguousarray(ps.miss_cull_boxes())
    dl = ps.direct_lists()
    print(f"{scene}: {len(boxes)} occluder boxes, triangles per box {dl['box_tris'].tolist()}, product K = {dl['k']}")
    if not len(boxes):
        print("  no boxes: no miss cull, no lists")
        return
    s = oracle.Scene(path)
    for k in ks:
        counts, lists = lists_for(dl, k if k else dl["k"])
        if not k:   # the product's own lists: what the kernels get
            own = dl["list_kd"]
            assert np.array_equal(counts[: len(own)], dl["counts"].astype(np.int32))
            assert np.array_equal(lists[: len(own), : own.shape[1]], own)
        print(f"  K = {k if k else dl['k']}{'' if k else ' (the product lists)'}: listed boxes {np.flatnonzero(counts).tolist()}")
        L.diag_init(boxes.ctypes.data_as(C.POINTER(C.c_float)), len(boxes), counts.ctypes.data_as(ip),
                    np.ascontiguousarray(lists).ctypes.data_as(ip), 16)
        # the whole C2 view at size x size; one thread: the hooks' sums are global
        _, c = s.render(oracle.RenderParams(width=size, height=size, spp=spp, spp_chunk=spp, traversal=oracle.KD_ORDERED,
                                            threads=1))
        acc = (C.c_double * (16 * 8))()
        L.diag_read(acc)
        a = np.array(acc[:]).reshape(16, 8)
        print(f"    {size}x{size} x {spp} spp: rays {c['rays']}, secondary {int(a[:, 0].sum())}")
        print("    depth  secondary   walked   direct  of-walked  list != walk   inner/tests walked   inner/tests direct")
        for dpt in range(1, 16):
            n, w, dr, bad, i_w, t_w, i_d, t_d = a[dpt]
            if not n:
                continue
            print(f"    {dpt:5d} {int(n):10d} {int(w):8d} {int(dr):8d} {dr / max(w, 1):9.1%} {int(bad):13d}"
                  f"   {i_w / max(w, 1):9.1f} /{t_w / max(w, 1):5.1f}   {i_d / max(dr, 1):9.1f} /{t_d / max(dr, 1):5.1f}")
        n, w, dr, bad, i_w, t_w, i_d, t_d = a.sum(axis=0)
        print(f"    walked secondary rays {int(w)} ({int(n - w)} hit no box): {dr / max(w, 1):.1%} direct, {int(bad)} of them "
              f"with another hit id than the walk's; they hold {i_d / max(i_w, 1):.1%} of the walked rays' inner visits "
              f"and {t_d / max(t_w, 1):.1%} of their triangle tests")


if __name__ == "__main__":
    main()

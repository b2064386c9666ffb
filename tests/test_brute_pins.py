"""'Ordered KD walk (+ fp16 child-box cull) == brute force' where the product
relies on it, and the scene02 statistical pin.

Every GPU parity test compares the kernel with the oracle's ordered walk
(KD_ORDERED); for scenes served from global memory (C4's 70k-triangle mesh,
scenes 02/03) both sides also run the fp16 child-box cull.  Here that walk --
with the cull on and off -- is held to the brute-force restatement of
CUTracer.cu:44-96 (every geometry, every triangle, strict t < tmin, ties in
loop order) on 112 500 rays per scene (tests/_raysets.py ray_sets(., 100 000)):
25 000 random rays, 25 000 aimed at triangle interiors and 12 500 each of
axis-parallel rays, origins exactly on KD split planes, origins on triangle
edges, rays grazing a triangle's plane and rays through vertices.
Hits are compared bit for bit (triangle, geometry, beta, gamma, t, hit point).

scene02 pin: the reference's own MC.docx Figure 3 ("Scene 2 with luminance 10
and 10000 samples (Blinn-Phong model)", MC.docx para 62-67) is the current
code's sampler (Utils.hpp:72-95 samples the Blinn-Phong half vector).  Its
result2step/step000009.png is the *Phong-model* render of Figure 4 (para 64-68:
sampling around the mirror direction, a variant the shipped code does not
contain, with its camera 9 px lower): the test shows it agrees with Figure 4
and is rejected against the current code, as result1.png's current-code
variant is (tests/test_oracle.py).
"""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
THREADS = min(os.cpu_count() or 8, 16)


from _exact_hits import float_artifact as _float_artifact  # noqa: E402  (shared with test_ray_contract_cpu.py)
from _raysets import EDGE_ORIGINS, ray_sets as _ray_sets  # noqa: E402  (shared with the GPU query tests)


@pytest.fixture(scope="module")
def oscene(oracle_mod):
    from montecarlopathtracer_amd.scenes import scene_path
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle_mod.Scene(scene_path(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", ["scene02", "scene03", "cornell_bunny70k"])
def test_ordered_walk_and_box_cull_equal_brute_force(oscene, oracle_mod, name):
    """Bit-identical hits on every ray of the random, aimed, axis-parallel,
    split-plane-origin, grazing and through-vertex families.  Rays that start
    exactly on a triangle edge (family 5) may differ, and only where the
    reference's own float arithmetic is inconsistent (checked exactly): there
    the brute force accepts a triangle the exact test rejects, or orders two
    hits against their exact order -- hits no traversal that prunes by region
    can reproduce (the reference's own KD walk, rtx.hlsl:144-211, differs from
    its brute force on more of them)."""
    s = oscene(name)
    o, d, fam = _ray_sets(s, 100_000, seed=17, families=True)
    fam5 = fam == EDGE_ORIGINS                              # origins on triangle edges
    assert o.shape[0] >= 112_500 - 100 and (np.bincount(fam, minlength=8)[1:] >= 12_500 - 100).all()
    tb, gb, hb, cb = s.intersect(o, d, oracle_mod.BRUTE, threads=THREADS)
    assert 0.3 < (tb >= 0).mean() < 1.0
    kv = s.kd_verts()
    modes = [(oracle_mod.KD_ORDERED, 0), (oracle_mod.KD_ORDERED, 1)]
    for mode, boxes in modes:
        tk, gk, hk, ck = s.intersect(o, d, mode, node_boxes=boxes, threads=THREADS)
        bad = np.nonzero((tb != tk) | (gb != gk) | (hb.view(np.uint32) != hk.view(np.uint32)).any(axis=1))[0]
        assert not (~fam5[bad]).any(), (name, boxes, bad[~fam5[bad]][:10])
        assert bad.size <= 50, (name, boxes, bad.size)
        for i in bad:
            assert _float_artifact(kv, o[i], d[i], tb[i], hb[i], tk[i], hk[i]), (name, boxes, i, tb[i], tk[i])
        assert ck["tri_tests"] < 0.05 * cb["tri_tests"]
    # the cull is what prunes: fewer inner visits and triangle tests than the plain walk
    _, _, _, c0 = s.intersect(o[:20000], d[:20000], oracle_mod.KD_ORDERED, node_boxes=0, threads=THREADS)
    _, _, _, c1 = s.intersect(o[:20000], d[:20000], oracle_mod.KD_ORDERED, node_boxes=1, threads=THREADS)
    assert c1["tri_tests"] <= c0["tri_tests"] and c1["inner_visits"] <= c0["inner_visits"]


def test_bunny_image_brute_equals_ordered_with_boxes(oscene, oracle_mod):
    """C4 mesh image: brute force (CUTracer.cu:44-96) and the kernel's walk with
    the child-box cull render the same pixels with the same ray and shade counts."""
    s = oscene("cornell_bunny70k")
    kw = dict(width=32, height=24, spp=2, threads=THREADS)
    a, ca = s.render(oracle_mod.RenderParams(traversal=oracle_mod.BRUTE, **kw))
    b, cb = s.render(oracle_mod.RenderParams(traversal=oracle_mod.KD_ORDERED, node_boxes=1, **kw))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert ca["rays"] == cb["rays"] and ca["shades"] == cb["shades"] and ca["paths"] == cb["paths"]
    assert a.max() > 0


def _blocks_vs_figure(img800, fig):
    """8-bit encode an 800x600 render, scale it to the figure's 607x455, and
    compare 75x75 block means on the 600x450 crop where the figure is not saturated."""
    from PIL import Image
    enc = np.clip(np.rint(img800 * 255), 0, 255).astype(np.uint8)
    ours = np.asarray(Image.fromarray(enc).resize(fig.shape[1::-1], Image.BILINEAR)).astype(np.float32) / 255
    B = lambda a: a[:450, :600].reshape(6, 75, 8, 75, 3).mean(axis=(1, 3))  # noqa: E731
    unsat = ~((fig[:450, :600] >= 250 / 255).reshape(6, 75, 8, 75, 3).any(axis=(1, 3, 4)))
    return np.abs(B(ours) - B(fig))[unsat]


def load_png(name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(GOLDEN, name)).convert("RGB")).astype(np.float32) / 255


def test_scene02_statistical_pin_against_mcdocx_figure3(oscene, oracle_mod):
    s = oscene("scene02")
    img, _ = s.render(oracle_mod.RenderParams(width=800, height=600, spp=32, illum=10.0, scene_id=2,
                                              traversal=oracle_mod.KD_ORDERED, node_boxes=1, threads=THREADS))
    d3 = _blocks_vs_figure(img, load_png("mcdocx_fig3_scene2_blinn_phong.png"))
    assert d3.size >= 30 and d3.mean() < 0.007 and d3.max() < 0.012, (d3.mean(), d3.max())
    d4 = _blocks_vs_figure(img, load_png("mcdocx_fig4_scene2_phong.png"))
    assert d4.max() > 0.025, d4.max()                     # the Phong-model figure is another sampler
    # result2step/step000009.png (1000 spp) is that Phong-model render: close to Figure 4,
    # far from Figure 3 and from the current code
    step = load_png("result2_step000009.png")
    assert _blocks_vs_figure(step, load_png("mcdocx_fig4_scene2_phong.png")).mean() < 0.006
    assert _blocks_vs_figure(step, load_png("mcdocx_fig3_scene2_blinn_phong.png")).mean() > 0.01


@pytest.mark.parametrize("name", ["scene01", "scene02", "scene03"])
def test_sah_tree_walk_equals_brute_force(oracle_mod, name):
    """The opt-in SAH tree (kd_build "sah": region SAH, triangles assigned by
    their boxes clipped to the node region) under the same adversarial ray
    families: the ordered walk, with the child-box cull on and off, returns
    the brute-force hit bit for bit except the float artifacts of rays that
    start on a triangle edge (family 5), as for the reference tree."""
    from montecarlopathtracer_amd.scenes import scene_path
    s = oracle_mod.Scene(scene_path(name), kd_build="sah")
    o, d, fam = _ray_sets(s, 60_000, seed=23, families=True)
    fam5 = fam == EDGE_ORIGINS
    tb, gb, hb, _ = s.intersect(o, d, oracle_mod.BRUTE, threads=THREADS)
    kv = s.kd_verts()
    for boxes in (0, 1):
        tk, gk, hk, _ = s.intersect(o, d, oracle_mod.KD_ORDERED, node_boxes=boxes, threads=THREADS)
        bad = np.nonzero((tb != tk) | (gb != gk) | (hb.view(np.uint32) != hk.view(np.uint32)).any(axis=1))[0]
        assert not (~fam5[bad]).any(), (name, boxes, bad[~fam5[bad]][:10])
        for i in bad:
            assert _float_artifact(kv, o[i], d[i], tb[i], hb[i], tk[i], hk[i]), (name, boxes, i, tb[i], tk[i])

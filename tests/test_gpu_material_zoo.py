"""The material-ends scenes (tests/_matzoo.py) on the GPU, against the CPU oracle.

edges and nanfloor: both pipelines, the wavefront in queue order and sorted, lean and
counting, both layouts -- image bit for bit (and finite: a NaN ray misses and stores 0),
`rays`, `paths`, `shades`, and for the megakernel and the counting wavefront the
oracle's visit counters, so the NaN rays nanfloor's floor makes (tests/
test_material_zoo_cpu.py counts them) are walked as the oracle walks them: to one leaf,
nothing pushed, no hit ("NaN rays").  QuinEngine mode, repeated
renders, radiance queries on the frame's own primary rays and the feature buffers'
albedo run on the same scenes.

gain20 / gain18 / gain19: the terminal cull's admission rule (plan.cpp: the cull stores 0
where the reference stores throughput * 0, so it is off once
log2(max(1, cull_gain)) * max_depth >= 127, when the throughput can be inf).  gain20's
NaN pixels must be the oracle's; gain18 (18 * 7 = 126) still culls at depth 7, gain19
(19 * 7 = 133) must not.

Frames are test_gpu_zoo's: 64 x 64 and 48 x 64 px, 5 spp in chunks of 2, tile 8, from
ZOO_CAM; every render is at most 20 480 paths.
"""
import numpy as np
import pytest

import _aov_ref as A
from _matzoo import matzoo_scenes, same_nan_aware  # noqa: F401  (matzoo_scenes: a fixture)
from _zoo import ZOO_CAM
from test_gpu_edge_scenes import COUNTS
from test_gpu_radiance import SEED, combine, query
from test_gpu_zoo import CHUNK, DEPTHS, FRAMES, KEYS, _check, _params
from test_miss_cull import _same

pytestmark = pytest.mark.gpu

NAN_SCENES = ("edges", "nanfloor")
QE_DEPTH, QE_SEED = 5, 0x5EED


@pytest.fixture(scope="module")
def mz_oracle(oracle_mod, matzoo_scenes):  # noqa: F811
    """(scene, frame, depth, node_boxes, mode) -> the oracle's (image, counters), rendered once and read-only"""
    have, scenes = {}, {}

    def scene(name):
        if name not in scenes:
            scenes[name] = oracle_mod.Scene(matzoo_scenes[name])
        return scenes[name]

    def get(name, frame, depth, boxes=0, qe=False):
        key = (name, frame, depth, boxes, qe)
        if key not in have:
            w, h, spp = FRAMES[frame]
            kw = dict(ZOO_CAM)
            if qe:
                kw.update(mode=oracle_mod.MODE_QE, seed=QE_SEED, illum=1.0, fov=45.0, fresnel_kd=0)
            img, cnt = scene(name).render(oracle_mod.RenderParams(
                width=w, height=h, spp=spp, spp_chunk=CHUNK, max_depth=depth, threads=16, node_boxes=boxes, **kw))
            img.setflags(write=False)
            have[key] = (img, cnt)
        return have[key]

    get.scene = scene
    return get


@pytest.fixture(scope="module")
def mz_gpu(mcpt, matzoo_scenes):  # noqa: F811
    """(scene, layout) -> the scene on the device, made once"""
    have = {}

    def get(name, layout="auto"):
        if (name, layout) not in have:
            have[name, layout] = mcpt.Scene(mcpt.ObjModel(matzoo_scenes[name]), layout=layout)
            assert have[name, layout].info()["node_boxes"] == (1 if layout == "global" else 0)
        return have[name, layout]

    yield get
    for s in have.values():
        s.close()


def _mega(mcpt, frame, depth):
    w, h, spp = FRAMES[frame]
    return mcpt.RenderParams(width=w, height=h, spp=spp, spp_chunk=CHUNK, tile=8, max_depth=depth, pipeline="megakernel",
                             **ZOO_CAM)


def _qe(mcpt, frame, **kw):
    w, h, spp = FRAMES[frame]
    return mcpt.RenderParams.for_quinengine(width=w, height=h, spp=spp, spp_chunk=CHUNK, tile=8, max_depth=QE_DEPTH,
                                            seed=QE_SEED, **ZOO_CAM, **kw)


def _counts_equal(st, rc, what):
    for k in COUNTS:
        assert st[k] == rc[k], (what, k, st[k], rc[k])


# ---- edges and nanfloor -------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["auto", "global"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("name", NAN_SCENES)
def test_matches_oracle(mcpt, mz_oracle, mz_gpu, name, frame, depth, layout):
    scene = mz_gpu(name, layout)
    boxes = int(layout == "global")
    ref, rc = mz_oracle(name, frame, depth, boxes)
    assert np.isfinite(ref).all() and float(ref.max()) > 0.0 and rc["shades"] > 0
    img, st = scene.render(_mega(mcpt, frame, depth))
    assert _same(img, ref), "megakernel"
    _counts_equal(st, rc, "megakernel")
    for sort in (False, True):
        ls = _check(mcpt, scene, ref, rc, frame, depth, sort=sort)     # lean = counting = oracle; the lean inequalities
        full, fs = scene.render(_params(mcpt, frame, depth, lean=False, sort=sort))
        assert _same(full, ref)
        _counts_equal(fs, rc, ("wavefront", sort))
        if layout == "auto":                                           # in LDS: the lists are on (nanfloor is panes:
            assert scene.info()["direct_list_boxes"] > 0               # test_gpu_zoo._extras)
            assert name != "nanfloor" or ls["direct_rays"] > 0


@pytest.mark.parametrize("layout", ["auto", "global"])
@pytest.mark.parametrize("name", NAN_SCENES)
def test_quinengine_mode_matches_oracle(mcpt, mz_oracle, mz_gpu, name, layout):
    """rtx.hlsl semantics on the same materials: the float Ns (Ns 1.5: exponent 1 / 2.5), every
    Fresnel output through HLSL normalize -- a NaN direction stays NaN"""
    scene = mz_gpu(name, layout)
    ref, rc = mz_oracle(name, "a", QE_DEPTH, int(layout == "global"), qe=True)
    assert np.isfinite(ref).all() and float(ref.max()) > 0.0
    img, st = scene.render(_qe(mcpt, "a", pipeline="megakernel"))
    assert _same(img, ref), "megakernel"
    _counts_equal(st, rc, "megakernel")
    for sort in (False, True):
        full, fs = scene.render(_qe(mcpt, "a", pipeline="wavefront", wf_sort=sort, lean=False))
        assert _same(full, ref), sort
        _counts_equal(fs, rc, ("wavefront", sort))
        lean, ls = scene.render(_qe(mcpt, "a", pipeline="wavefront", wf_sort=sort, lean=True))
        assert _same(lean, ref), sort
        assert ls["rays"] == rc["rays"] and ls["paths"] == rc["paths"] and ls["shades"] == rc["shades"]


@pytest.mark.parametrize("name", NAN_SCENES)
def test_two_renders_are_bit_identical(mcpt, mz_gpu, name):
    scene = mz_gpu(name)
    a, sa = scene.render(_params(mcpt, "a", 7))
    b, sb = scene.render(_params(mcpt, "a", 7))
    assert _same(a, b)
    assert {k: sa[k] for k in KEYS} == {k: sb[k] for k in KEYS}


@pytest.mark.parametrize("layout", ["auto", "global"])
@pytest.mark.parametrize("name", NAN_SCENES)
def test_radiance_queries_on_the_frames_primary_rays_give_the_render(mcpt, oracle_mod, mz_oracle, mz_gpu, name, layout):
    """the render's primary rays, queried sample by sample and summed as the kernels sum"""
    w, h, spp = FRAMES["b"]
    scene = mz_gpu(name, layout)
    ref, _ = mz_oracle(name, "b", 7, int(layout == "global"))
    samples = []
    for s in range(spp):
        o, d = A.primary_rays(oracle_mod, w, h, 1, spp_offset=s, seed=SEED, eye=ZOO_CAM["eye"],
                              direction=ZOO_CAM["direction"])
        samples.append(query(scene, o, d, spp=1, spp_offset=s, max_depth=7, fresnel_kd=1, seed=SEED))
    got = combine(samples, CHUNK).reshape(h, w, 3)
    assert _same(got, ref)


@pytest.mark.parametrize("fresnel_kd", [0, 1])
def test_edges_albedo_matches_restatement(mcpt, oracle_mod, mz_oracle, mz_gpu, fresnel_kd):
    """the feature buffers' albedo by class: Kd for Ns exactly 1 (its Ks line is dead), Ks for Ns 1.5 and
    the coloured Ks, Kd 2 unclamped, 1 for the emitting glass"""
    w, h, spp = FRAMES["a"]
    for layout in ("auto", "global"):
        ac, nd = mz_gpu("edges", layout).render_aov(mcpt.RenderParams(width=w, height=h, spp=spp, fresnel_kd=bool(fresnel_kd),
                                                                     **ZOO_CAM))
        rac, rnd = A.aov_reference(oracle_mod, mz_oracle.scene("edges"), w, h, spp, node_boxes=int(layout == "global"),
                                   fresnel_kd=bool(fresnel_kd), eye=ZOO_CAM["eye"], direction=ZOO_CAM["direction"])
        assert _same(ac, rac) and _same(nd, rnd), layout
        assert float(ac[..., 0].max()) > 1.0                            # Kd 2 is seen


# ---- the gain scenes ------------------------------------------------------------------------------

def _renders(mcpt, scene, frame, depth):
    """name -> (image, stats): the megakernel, and the wavefront in queue order and sorted, lean and counting"""
    out = {"megakernel": scene.render(_mega(mcpt, frame, depth))}
    for sort in (False, True):
        for lean in (True, False):
            out["wavefront-%s-%s" % ("sorted" if sort else "queue", "lean" if lean else "counting")] = scene.render(
                _params(mcpt, frame, depth, lean=lean, sort=sort))
    return out


@pytest.mark.parametrize("layout", ["auto", "global"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_gain20_keeps_the_oracles_nan_pixels(mcpt, mz_oracle, mz_gpu, depth, layout):
    """Kd 1e20: log2(1e20) * 2 = 132.9 >= 127, so from depth 2 on no render may cull a terminal ray -- a culled one
    stores 0 where the reference's inf * 0 is NaN.  Oracle, 64 x 64: 0 / 269 / 751 / 25 NaN pixels at depths
    1 / 2 / 3 / 7.  At depth 1 (66.4 < 127) the cull is on and the image finite"""
    ref, rc = mz_oracle("gain20", "a", depth, int(layout == "global"))
    nan = int(np.isnan(ref).any(axis=2).sum())
    print("gain20 depth %d: %d NaN pixels in the oracle's image" % (depth, nan))
    assert (nan == 0) == (depth == 1)
    for what, (img, st) in _renders(mcpt, mz_gpu("gain20", layout), "a", depth).items():
        assert int(np.isnan(img).any(axis=2).sum()) == nan, what
        assert same_nan_aware(img, ref), what
        if depth == 1:
            assert _same(img, ref), what
        assert st["rays"] == rc["rays"] and st["paths"] == rc["paths"] and st["shades"] == rc["shades"], what


@pytest.mark.parametrize("layout", ["auto", "global"])
def test_gain18_culls_terminal_rays_and_gain19_does_not(mcpt, mz_oracle, mz_gpu, layout):
    """Depth 7, Kd 2^18 and 2^19 either side of the rule; both images are finite and the oracle's.  The three
    scenes trace the same rays (tests/test_material_zoo_cpu.py), so their lean renders' counters tell what the
    culls did: gain19's secondary rays have the fates of its twin's, a scene without emitter boxes that can cull
    no terminal ray; gain18's walked and resolved rays are fewer -- its terminal cull dropped the difference.
    (test_terminal_cull.py states no margin for scene01's cull and no counter relation for its `negative` scene;
    the strict inequality and the twin stand in for them.)  Measured: of 33 235 secondary rays gain19 and its twin
    walk or resolve 22 174, gain18 22 158 in LDS and 22 124 from global memory"""
    fate = {}
    for name in ("gain18", "gain19", "gain19_nocull"):
        ref, rc = mz_oracle(name, "a", 7, int(layout == "global"))
        assert np.isfinite(ref).all()
        for what, (img, st) in _renders(mcpt, mz_gpu(name, layout), "a", 7).items():
            assert _same(img, ref), (name, what)
            assert st["rays"] == rc["rays"] and st["paths"] == rc["paths"] and st["shades"] == rc["shades"], (name, what)
            if what.endswith("lean"):
                fate[name, what] = {k: st[k] for k in KEYS}
            elif what.endswith("counting"):
                assert st["extend_rays"] == rc["rays"] - rc["paths"], (name, what)
    for what in ("wavefront-queue-lean", "wavefront-sorted-lean"):
        g18, g19, twin = fate["gain18", what], fate["gain19", what], fate["gain19_nocull", what]
        secondary = g19["rays"] - g19["paths"]
        print("%s %s: secondary %d; extend + direct: gain18 %d, gain19 %d, no emitter boxes %d" % (
            layout, what, secondary, g18["extend_rays"] + g18["direct_rays"], g19["extend_rays"] + g19["direct_rays"],
            twin["extend_rays"] + twin["direct_rays"]))
        assert g19 == twin, what
        assert g18["rays"] == g19["rays"] and g18["paths"] == g19["paths"]
        assert g18["extend_rays"] + g18["direct_rays"] < g19["extend_rays"] + g19["direct_rays"] <= secondary, what

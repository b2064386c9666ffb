"""The scene zoo (tests/_zoo.py) on the GPU: the lean wavefront's miss cull, direct
resolve and clip walk on scenes whose occluder boxes differ from scene01's --
lists of one triangle (single), clip intervals joined over up to five unlisted
boxes with gaps and overlaps (tetras), listed boxes of glass and mirror with full
walks beside clipped ones (panes), thick boxes merged around empty space (many).
tests/test_zoo_cpu.py holds the scenes' structure and counts, on the oracle's own
rays, the rays that take each of these branches.

The oracle (which walks every ray in full) is the reference everywhere: the lean
render and the counting render (no culls, no lists, no selectors) must give its
image bit for bit and its `rays`, `paths` and `shades`.  Frames are 64 x 64 and
48 x 64 px, 5 spp in chunks of 2, tile 8, from eye (0, 5, 7) towards (0, -0.3, -1)
unless a test says otherwise.
"""
import numpy as np
import pytest

from _zoo import SINGLE_CAM_BELOW, TETRAS, TETRAS_MIDDLE, ZOO, ZOO_CAM, zoo_scenes  # noqa: F401  (zoo_scenes: a fixture)
from test_miss_cull import _same

CHUNK = 2
FRAMES = {"a": (64, 64, 5), "b": (48, 64, 5)}       # width, height, spp
DEPTHS = (1, 2, 3, 7)
KEYS = ("rays", "paths", "shades", "direct_rays", "extend_rays", "clipped_rays")


@pytest.fixture(scope="module")
def zoo_oracle(oracle_mod, zoo_scenes):  # noqa: F811
    """(scene, frame, depth, camera, mode) -> the oracle's (image, counters), rendered once and read-only"""
    have, scenes = {}, {}

    def get(name, frame, depth, cam=ZOO_CAM, qe=False):
        key = (name, frame, depth, tuple(sorted(cam.items())), qe)
        if key not in have:
            if name not in scenes:
                scenes[name] = oracle_mod.Scene(zoo_scenes[name])
            w, h, spp = FRAMES[frame]
            kw = dict(cam)
            if qe:
                kw.update(mode=oracle_mod.MODE_QE, seed=0x5EED, illum=1.0, fov=45.0, fresnel_kd=0)
            img, cnt = scenes[name].render(oracle_mod.RenderParams(
                width=w, height=h, spp=spp, spp_chunk=CHUNK, max_depth=depth, threads=16, **kw))
            img.setflags(write=False)
            have[key] = (img, cnt)
        return have[key]

    return get


@pytest.fixture(scope="module")
def zoo_gpu(mcpt, zoo_scenes):  # noqa: F811
    """(scene, layout) -> the scene on the device, made once"""
    have = {}

    def get(name, layout="auto"):
        if (name, layout) not in have:
            have[name, layout] = mcpt.Scene(mcpt.ObjModel(zoo_scenes[name]), layout=layout)
        return have[name, layout]

    yield get
    for s in have.values():
        s.close()


def _params(mcpt, frame, depth, lean=True, sort=False, cam=ZOO_CAM):
    w, h, spp = FRAMES[frame]
    return mcpt.RenderParams(width=w, height=h, spp=spp, spp_chunk=CHUNK, tile=8, max_depth=depth,
                             pipeline="wavefront", wf_sort=sort, lean=lean, **cam)


def _check(mcpt, scene, ref, rc, frame, depth, sort=False, cam=ZOO_CAM):
    """lean = counting = oracle: image bits, rays, paths and shades; the counting render resolves and
    clips nothing and its extends take every secondary ray; the lean render's direct and walked rays
    are among the secondary rays, its clipped rays among the walked ones; -> the lean stats"""
    lean, ls = scene.render(_params(mcpt, frame, depth, sort=sort, cam=cam))
    full, fs = scene.render(_params(mcpt, frame, depth, lean=False, sort=sort, cam=cam))
    print("depth %d: rays %d, paths %d, direct %d, extend %d, clipped %d" %
          (depth, ls["rays"], ls["paths"], ls["direct_rays"], ls["extend_rays"], ls["clipped_rays"]))
    assert _same(lean, ref) and _same(full, ref)
    for st in (ls, fs):
        assert st["rays"] == rc["rays"] and st["paths"] == rc["paths"] and st["shades"] == rc["shades"]
    assert fs["direct_rays"] == 0 == fs["clipped_rays"]
    assert fs["extend_rays"] == rc["rays"] - rc["paths"]
    assert ls["extend_rays"] + ls["direct_rays"] <= rc["rays"] - rc["paths"]
    assert 0 <= ls["clipped_rays"] <= ls["extend_rays"]
    return ls


def _extras(name, depth, ls):
    """what each scene is for, in the lean render's counters"""
    if name == "single":                   # every direct ray went through a list of one triangle
        assert ls["direct_rays"] > 0
        if depth >= 2:
            assert ls["clipped_rays"] > 0
    elif name == "tetras":                 # only the light is listed (measured: every walked ray is clipped)
        if depth >= 2:
            assert ls["clipped_rays"] > 0.5 * ls["extend_rays"]
    elif name == "panes":                  # rays through two listed boxes walk in full beside clipped ones
        assert ls["direct_rays"] > 0
        if depth >= 2:
            assert 0 < ls["clipped_rays"] < ls["extend_rays"]
    elif name == "many":
        if depth >= 2:
            assert ls["direct_rays"] > 0 and ls["clipped_rays"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("name", ZOO)
def test_matches_oracle(mcpt, zoo_oracle, zoo_gpu, name, frame, depth, sort):
    """depth 1's only secondary rays are the terminal query's: a direct one's emission (single: the
    one-triangle emitter's) is stored by the shade's resolve"""
    scene = zoo_gpu(name)
    assert scene.info()["node_boxes"] == 0 and scene.info()["direct_list_boxes"] > 0
    ref, rc = zoo_oracle(name, frame, depth)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    _extras(name, depth, _check(mcpt, scene, ref, rc, frame, depth, sort=sort))


def test_single_depth_1_shows_the_resolved_emission(zoo_oracle):
    """the precondition of depth 1's comparison: pixels that are black without secondary rays are lit
    by the terminal query's hit on the emitting triangle"""
    d0, d1 = zoo_oracle("single", "a", 0)[0], zoo_oracle("single", "a", 1)[0]
    lit = (d0.max(axis=2) == 0.0) & (d1.max(axis=2) > 0.0)
    print("pixels lit by depth 1 alone:", int(lit.sum()))
    assert lit.sum() >= 100


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_single_quinengine(mcpt, zoo_oracle, zoo_gpu, sort):
    depth = 2
    ref, rc = zoo_oracle("single", "a", depth, qe=True)
    assert float(ref.max()) > 0.0
    scene = zoo_gpu("single")
    w, h, spp = FRAMES["a"]
    for lean in (True, False):
        img, st = scene.render(mcpt.RenderParams.for_quinengine(
            width=w, height=h, spp=spp, spp_chunk=CHUNK, tile=8, max_depth=depth, seed=0x5EED, pipeline="wavefront",
            wf_sort=sort, lean=lean, **ZOO_CAM))
        assert _same(img, ref) and st["rays"] == rc["rays"], lean
        assert (st["direct_rays"] > 0) == lean and (st["clipped_rays"] > 0) == lean
        assert st["clipped_rays"] <= st["extend_rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
@pytest.mark.parametrize("depth", [1, 3])
def test_single_triangle_fills_the_frame(mcpt, zoo_oracle, zoo_gpu, depth, sort):
    """from below and in front of the lone red triangle: nine first hits in ten are on it, and the
    rays that leave it start inside its one-triangle box"""
    ref, rc = zoo_oracle("single", "a", depth, cam=SINGLE_CAM_BELOW)
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    ls = _check(mcpt, zoo_gpu("single"), ref, rc, "a", depth, sort=sort, cam=SINGLE_CAM_BELOW)
    assert ls["direct_rays"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("sort", [False, True], ids=["queue", "sorted"])
def test_tetras_eye_inside_an_object_box(mcpt, zoo_oracle, zoo_gpu, sort):
    """the eye at the centre of the middle tetrahedron: the first hits are inside it, so the rays that
    leave them start inside their unlisted box and its slab interval begins at 0"""
    scene = zoo_gpu("tetras")
    c = np.array(TETRAS[TETRAS_MIDDLE][0], np.float32)
    b = scene.miss_cull_boxes()
    inside = ((b[:, :3] < c) & (c < b[:, 3:])).all(axis=1) & (scene.direct_lists()["box_tris"] == 4)
    assert inside.sum() == 1
    b = b[inside][0]
    cam = dict(eye=tuple(float(x) for x in (b[:3] + b[3:]) / 2), direction=(0.3, -0.2, -1.0))
    ref, rc = zoo_oracle("tetras", "a", 3, cam=cam)
    assert rc["shades"] > 0
    ls = _check(mcpt, scene, ref, rc, "a", 3, sort=sort, cam=cam)
    assert ls["clipped_rays"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ZOO)
def test_global_layout_keeps_the_full_walk(mcpt, zoo_oracle, zoo_gpu, name):
    scene = zoo_gpu(name, "global")
    assert scene.info()["node_boxes"] == 1
    ref, rc = zoo_oracle(name, "a", 3)
    ls = _check(mcpt, scene, ref, rc, "a", 3)
    assert ls["direct_rays"] == 0 == ls["clipped_rays"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ZOO)
def test_two_renders_are_bit_identical(mcpt, zoo_gpu, name):
    """queue order depends on scheduling; nothing reads it, and what becomes of a ray depends on the ray alone"""
    scene = zoo_gpu(name)
    a, sa = scene.render(_params(mcpt, "a", 7))
    b, sb = scene.render(_params(mcpt, "a", 7))
    assert _same(a, b)
    assert {k: sa[k] for k in KEYS} == {k: sb[k] for k in KEYS}

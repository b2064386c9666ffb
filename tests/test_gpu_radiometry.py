"""The HIP kernels against closed-form radiometry (tests/_radiometry.py): what
tests/test_radiometry_cpu.py asks the CPU oracle, asked of the radiance queries,
the megakernel, the wavefront pipelines and QuinEngine mode.  The kernels equal
the oracle bit for bit (every other module), and the oracle carries the same
float expressions; only a closed form says whether they compute the right thing.

Queries: R = 4096 copies of the case's one ray with stream ids 0 .. R-1, 1024
samples each, N = 2^22 samples of one Bernoulli variable of known probability p,
the library's default seed.  Asserted per case, at depth 1 and 7, with the scene
in LDS and in global memory: the lean and the counting kernel give equal bits; the
per-ray counts are integers, equal in the channels; |k - N p| <= 5 sqrt(N p (1 - p));
the variance of the per-ray counts over S p (1 - p) within 1 +- 5 sqrt(2 / (R - 1)); the
lag-1 autocorrelation of the counts over the stream id within 5 / sqrt R; where every
sample has one exact value (dome, pane totals, total internal reflection) at most
16 in 2^20 differ.  At N = 2^22 the z-test resolves a relative error in p of
5 sqrt((1 - p) / (N p)): 0.9 % at p = 0.07 (plates), 0.7 % at p = 0.1 (pane up to 60
degrees), 0.4 % at p = 0.3 (Phong, Ns 10), 0.3 % at 0.45 (pane 80, Phong Ns 1000),
0.1 % (of 1 - p) at the pane's 88 degrees.

Renders: the narrow camera of the CPU module, 32 x 32 px, 256 spp (N = 2^18, four
times those figures), four pipelines with equal bits; QuinEngine mode over 256
frames.  The new scenes also render against the oracle bit for bit, counters
included: they pair walls 2000 units wide with objects of 2.

Each test prints its figures (profiles/radiometry/z_table.md is made of them).
"""
import numpy as np
import pytest

import _radiometry as R
from _radiometry import radiometry_scenes  # noqa: F401  (a fixture)
from test_gpu_radiance import COUNTERS, query, same
from test_radiometry_cpu import QeView, camera, check_counts

pytestmark = pytest.mark.gpu

RAYS, SPP = 4096, 1024
N = RAYS * SPP
RENDER_SPP = 256
RENDER_CASES = ("P1", "P3", "pane-front60-fkd1", "phong10", "dome-down")
QE_CASES = ("P1", "pane-front60-fkd0")
QE_FRAMES = 256
PIPELINES = (dict(pipeline="megakernel"), dict(pipeline="wavefront"), dict(pipeline="wavefront", lean=True),
             dict(pipeline="wavefront", wf_sort=True))


@pytest.fixture(scope="module")
def world(mcpt, oracle_mod, radiometry_scenes):  # noqa: F811
    """(scene name, layout) -> (device scene, oracle scene, geometry), each made once"""
    dev, orc = {}, {}

    def get(name, layout="auto"):
        if name not in orc:
            s = oracle_mod.Scene(radiometry_scenes[name])
            orc[name] = (s, R.Geometry(s))
        if (name, layout) not in dev:
            dev[name, layout] = mcpt.Scene(mcpt.ObjModel(radiometry_scenes[name]), layout=layout)
        return (dev[name, layout],) + orc[name]

    yield get
    for s in dev.values():
        s.close()


@pytest.mark.parametrize("layout", ["auto", "global"])
@pytest.mark.parametrize("depth", [1, 7])
@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_query_against_the_closed_form(world, case, depth, layout):
    """N = 2^22 samples of the case's one ray.  The z-test resolves a relative error of p of
    5 sqrt((1 - p) / (N p)): plates P1, P3..P6 (p 0.081..0.091) 0.8 %, P2 (0.183) 0.5 %, P7 (0.068) and P8 (0.072) 0.9 %;
    pane, of the reflected share: 0, 30, back 20 and back 41 degrees (0.100) 0.7 %, 60 (0.128) 0.6 %, 80 (0.447) 0.3 %,
    88 (0.854; of the transmitted 0.146) 0.6 %; Phong Ns 10 (0.304) 0.4 %, Ns 1000 (0.458) 0.3 %.  Back 43 and
    70 degrees and the dome are counting statements: at most 64 of the 2^22 samples may differ."""
    scene, _, geo = world(case.scene, layout)
    assert scene.info()["node_boxes"] == (layout == "global")
    o, d = case.ray()
    p = float(case.p_at(geo, o, d)[0])
    O, D, ids = np.tile(o, (RAYS, 1)), np.tile(d, (RAYS, 1)), np.arange(RAYS, dtype=np.uint32)
    kw = dict(spp=SPP, max_depth=depth, illum=case.illum, fresnel_kd=case.fresnel_kd)
    scene.trace_stats()
    got = query(scene, O, D, ids=ids, **kw)
    st = scene.trace_stats()
    assert same(query(scene, O, D, ids=ids, lean=1, **kw), got)
    assert st["paths"] == N
    if case.kind == "exact":
        assert st["rays"] == 2 * st["paths"]
    where = "query %s depth %d" % ("lds" if layout == "auto" else "global", depth)
    check_counts(case, got.reshape(RAYS, 1, 3), SPP, p, where)


def _render_params(mcpt, case, depth, **kw):
    return mcpt.RenderParams(width=R.PX, height=R.PX, spp=RENDER_SPP, max_depth=depth, illum=case.illum,
                             fresnel_kd=bool(case.fresnel_kd), fov_deg=case.fov, eye=tuple(case.eye),
                             direction=tuple(case.direction), up=case.up, **kw)


@pytest.mark.parametrize("depth", [1, 7])
@pytest.mark.parametrize("name", RENDER_CASES)
def test_render_against_the_closed_form(mcpt, oracle_mod, world, name, depth):
    """N = 2^18 samples over the narrow camera's 1024 pixels; the z-test resolves P1 and P3 (p 0.083) to
    3.2 %, the pane at 60 degrees (0.128) to 2.6 %, Phong Ns 10 (0.304) to 1.5 %; the dome counts (at most 4 differ)"""
    case = R.CASE[name]
    scene, _, geo = world(case.scene)
    n = R.PX * R.PX * RENDER_SPP
    _, cam = camera(oracle_mod, case)
    p = R.render_expectation(case, geo, cam, n)
    first = None
    for kw in PIPELINES:
        img, st = scene.render(_render_params(mcpt, case, depth, **kw))
        if first is None:
            first = img
            assert st["paths"] == n
            if case.kind == "exact":
                assert st["rays"] == 2 * st["paths"]
            check_counts(case, img, RENDER_SPP, p, "render depth %d" % depth)
        assert same(img, first), (name, kw)


@pytest.mark.parametrize("name", QE_CASES)
def test_quinengine_render_against_the_closed_form(mcpt, oracle_mod, world, name):
    """1 spp, depth 5, frame seeds 0 .. 255; each frame is gamma-encoded: a hit is a non-zero channel.
    N = 2^18: resolves P1 (p 0.083) to 3.2 %, the pane at 60 degrees (0.128) to 2.6 %"""
    case = R.CASE[name]
    scene, _, geo = world(case.scene)
    n = R.PX * R.PX * QE_FRAMES
    assert n >= 1 << 18
    _, cam = camera(oracle_mod, case, qe=True)
    p = R.render_expectation(case, geo, cam, n)
    hits = np.zeros((R.PX, R.PX, 3), np.float32)
    for seed in range(QE_FRAMES):
        frames = [scene.render(mcpt.RenderParams.for_quinengine(
            width=R.PX, height=R.PX, seed=seed, fov_deg=case.fov, eye=tuple(case.eye), direction=tuple(case.direction),
            up=case.up, pipeline=pipe))[0] for pipe in ("megakernel", "wavefront")]
        assert same(frames[0], frames[1]), seed
        hits += (frames[0] > 0)
    check_counts(QeView(case), hits / np.float32(QE_FRAMES), QE_FRAMES, p, "render quinengine")


@pytest.mark.parametrize("layout", ["auto", "global"])
@pytest.mark.parametrize("name", R.SCENES)
def test_new_scenes_match_the_oracle(mcpt, oracle_mod, world, name, layout):
    """32 x 24 px, 4 spp, the default field of view, the whole arrangement in view: image bits and
    counters of both pipelines, the lean and the sorted wavefront equal the oracle's"""
    scene, oscene, _ = world(name, layout)
    boxes = int(scene.info()["node_boxes"])
    assert boxes == (layout == "global")
    view = R.OVERVIEW[name]
    ref, rc = oscene.render(oracle_mod.RenderParams(width=32, height=24, spp=4, spp_chunk=2, threads=8, node_boxes=boxes,
                                                    traversal=oracle_mod.KD_ORDERED, **view))
    assert float(ref.max()) > 0.0 and rc["shades"] > 0
    for kw in PIPELINES:
        img, st = scene.render(mcpt.RenderParams(width=32, height=24, spp=4, spp_chunk=2, **view, **kw))
        assert same(img, ref), (name, kw)
        keys = COUNTERS if kw["pipeline"] == "megakernel" else ("rays", "paths", "shades")
        for k in keys:
            assert st[k] == rc[k], (name, kw, k, st[k], rc[k])

"""The ambient-occlusion and the direct-lighting kernels (csrc/ao.hip, csrc/direct.hip)
against closed-form radiometry (tests/_query_radiometry.py): what
tests/test_query_radiometry_cpu.py asks their numpy restatements, asked of the kernels with
16 times the samples.  test_gpu_ao.py and test_gpu_direct.py compare kernel and restatement
bit for bit, and the two share every float expression with include/mcpt.h; only a closed
form says whether g = cx cy A_tot / (pi r^2), the triangle warp, the area-weighted cdf, the
light's Ka, the emitter's |cos| and the rule origin = p + bias h, t < radius compute the right
thing.

Point forms: R = 4096 copies of the case's one point with stream ids 0 .. R-1, 1024 samples
each, N = 2^22, the library's default seed, each scene in LDS and in global memory (the fp16
child-box cull and the 256-thread kernels on scenes of 4 .. 6 triangles).  Asserted per case:
the lean and the counting call give equal bits; paths = N, and shades = rays = the samples that
formed a ray, N everywhere here; `check_ao` (the occluded count against N p, p a form factor
or the cap 1 - (h / (radius + bias))^2; a counting statement where p = 0) or `check_direct`
(the mean against E with the closed form's own sigma, per channel); both with the dispersion
of the per-stream values within 1 +- 5 sqrt(2 / (R - 1)) and their lag-1 autocorrelation within
5 / sqrt R.  At N = 2^22 the direct z-test resolves a relative error of E of 0.02 % (P5) to 0.1 %
(P8, L2's green), the AO one of p of 0.14 % (lid, radius 2) to 2.3 % (P8's blocker alone).
Variants: more than one chunk (dl_finish and the partial sums) and the 1024 samples as two
chained calls of 512 must pass the same checks.

Pixel forms: the narrow camera of test_radiometry_cpu.py, 32 x 32 px, 256 spp, N = 2^18 (four
times those figures); the expectation is the closed form's mean over the pixel centres' hit
points, guarded as R.render_expectation's.

A ray through a triangulation diagonal misses both triangles (the strict triangle test): at
most 16 in 2^20, so at most 64 of 2^22 AO samples against a sigma of about 560 counts, and for
the direct queries P8's blocker alone, a relative 1e-5 of the value -- below what the tests
resolve, and given no allowance of their own.

Each test prints its figures (profiles/radiometry/z_table.md is made of them).
"""
import numpy as np
import pytest

import _direct_ref as D
import _query_radiometry as Q
import _radiometry as R
from _query_radiometry import query_radiometry_scenes  # noqa: F401  (a fixture)
from _radiance_q import same
from _radiometry import radiometry_scenes  # noqa: F401  (a fixture)
from test_gpu_ao import ao_frame, ao_points
from test_gpu_direct import direct_frame, direct_points
from test_radiometry_cpu import camera

pytestmark = pytest.mark.gpu

POINTS, SPP = 4096, 1024
N = POINTS * SPP
PIXEL_SPP = 256
PIXEL_N = R.PX * R.PX * PIXEL_SPP
LAYOUTS = ["auto", "global"]


@pytest.fixture(scope="module")
def world(mcpt, oracle_mod, radiometry_scenes, query_radiometry_scenes):  # noqa: F811
    """(scene name, layout) -> (device scene, geometry, light table), each made once"""
    paths = dict(radiometry_scenes, **query_radiometry_scenes)
    dev, orc = {}, {}

    def get(name, layout="auto"):
        if name not in orc:
            s = oracle_mod.Scene(paths[name])
            orc[name] = (R.Geometry(s), D.light_table(s))
        if (name, layout) not in dev:
            dev[name, layout] = mcpt.Scene(mcpt.ObjModel(paths[name]), layout=layout)
        scene = dev[name, layout]
        assert scene.info()["node_boxes"] == (layout == "global")
        return (scene,) + orc[name]

    yield get
    for s in dev.values():
        s.close()


@pytest.fixture(scope="module")
def expected():
    """the closed forms' answers, each worked out once for both layouts"""
    memo = {}

    def get(key, make):
        if key not in memo:
            memo[key] = make()
        return memo[key]

    return get


def _copies(x, ns):
    return np.tile(x, (POINTS, 1)), np.tile(ns, (POINTS, 1)), np.arange(POINTS, dtype=np.uint32)


def _where(form, layout):
    return "%s %s" % (form, "lds" if layout == "auto" else "global")


# ---- the point forms ---------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", Q.DIRECT_POINT)
def test_direct_points_against_the_closed_form(world, expected, name, layout):
    """N = 2^22 samples at the case's one point, illum 2, the default bias.  The z-test resolves a relative error
    of E of 5 (sigma / E) / sqrt N: P5 (sigma / E 0.10) 0.024 %, P1, P3, P4, P6 (0.16 .. 0.17) 0.04 %, P7 (0.24) 0.06 %,
    L2 red (0.26) 0.06 %, P2 and L2 green and blue (0.39) and P8 (0.42) 0.1 %.  P2 sees the light's back (|ng . d|),
    P5 has n.y = 0, P7 takes the shading normal, P8's blocker hides 12 % of the light's area, L2's lights differ
    in area, distance and Ka."""
    scene, geo, table = world(name, layout)
    got_table = scene.lights()
    assert np.array_equal(got_table["kd_ids"], table["kd_ids"]) and same(got_table["cdf"], table["cdf"])
    assert same(got_table["normals"], table["normals"]) and got_table["area_total"] == table["area_total"]
    view = Q.View(name)
    x, ns = view.point(geo)
    E, var = expected(("direct", name), lambda: Q.direct_expectation(view, geo, table, x, ns))
    p, nrm, ids = _copies(x, ns)
    kw = dict(spp=SPP, illum=Q.ILLUM)
    scene.trace_stats()
    got = direct_points(scene, p, nrm, ids, **kw)
    st = scene.trace_stats()
    assert same(direct_points(scene, p, nrm, ids, lean=1, **kw), got)
    assert st["paths"] == N and st["shades"] == st["rays"] == N
    Q.check_direct(_where("direct point", layout), name, got, SPP, E, var)
    if name == "P1":
        # four chunks: the partial sums and dl_finish; the same expectation and sigma
        chunked = direct_points(scene, p, nrm, ids, spp_chunk=256, **kw)
        Q.check_direct(_where("direct point chunk 256", layout), name, chunked, SPP, E, var)
        # two chained calls of 512: for equal halves the running mean is the overall mean up to rounding
        first = direct_points(scene, p, nrm, ids, spp=SPP // 2, illum=Q.ILLUM)
        both = direct_points(scene, p, nrm, ids, prev=first, spp=SPP // 2, spp_offset=SPP // 2, prev_count=1,
                             illum=Q.ILLUM)
        assert not same(both, first)
        Q.check_direct(_where("direct point 2 x 512", layout), name, both, SPP, E, var)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", Q.AO_POINT, ids=Q.ao_id)
def test_ao_points_against_the_closed_form(world, expected, case, layout):
    """N = 2^22.  Resolves a relative error of p of 5 sqrt((1 - p) / (N p)): unbounded, p the light's form factor (P8's
    blocker lies inside the light): P1, P3 .. P6, P8 (0.081 .. 0.091) 0.8 %, P2 (0.183) 0.5 %, P7 (0.068) 0.9 %; the lid one
    unit above the point, bias 1 / 64: radius 2 (0.754) 0.14 %, 1.25 (0.376) 0.31 %, 1.0 (0.0305) 1.4 % -- measured from
    p, not from p + bias h, it would be exactly 0 -- and 0.96875: radius + bias < h, not one sample occluded; P8 at
    radius 6.5, the blocker alone within reach (0.0112) 2.3 %."""
    name, radius, bias = case
    scene, geo, _ = world(name, layout)
    view = Q.View(name)
    x, ns = view.point(geo)
    p_occ = expected(("ao",) + case, lambda: Q.ao_probability(view, geo, x, ns, radius, bias))
    p, nrm, ids = _copies(x, ns)
    kw = dict(spp=SPP, radius=radius, bias=bias)
    scene.trace_stats()
    got = ao_points(scene, p, nrm, ids, **kw)
    st = scene.trace_stats()
    assert same(ao_points(scene, p, nrm, ids, lean=1, **kw), got)
    assert st["paths"] == N and st["shades"] == st["rays"] == N
    Q.check_ao(_where("ao point", layout), Q.ao_id(case), got, SPP, p_occ)
    if case == ("lid", 1.25, 1 / 64):
        # two chained calls of 512: the halves' means are multiples of 1 / 512, their running mean is exact
        first = ao_points(scene, p, nrm, ids, spp=SPP // 2, radius=radius, bias=bias)
        both = ao_points(scene, p, nrm, ids, prev=first, spp=SPP // 2, spp_offset=SPP // 2, prev_count=1,
                         radius=radius, bias=bias)
        assert same(both, got)
        Q.check_ao(_where("ao point 2 x 512", layout), Q.ao_id(case), both, SPP, p_occ)


# ---- the pixel forms ---------------------------------------------------------------

def _frame_params(mcpt, view, **kw):
    return mcpt.RenderParams(width=R.PX, height=R.PX, spp=PIXEL_SPP, fov_deg=view.fov, eye=tuple(view.eye),
                             direction=tuple(view.direction), up=view.up, **kw)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", Q.DIRECT_PIXEL)
def test_direct_frame_against_the_closed_form(mcpt, oracle_mod, world, expected, name, layout):
    """N = 2^18 samples over the narrow camera's 1024 pixels: resolves 5 (sigma / E) / sqrt N, P1, P3, P6 0.16 %, P7 0.23 %,
    P8 0.41 %.  P6 is seen from behind (n = -nrm where dot(d, nrm) > 0), P7 shades with a normal off the face's."""
    scene, geo, table = world(name, layout)
    view = Q.View(name)
    _, cam = camera(oracle_mod, view)
    E, var = expected(("direct pixel", name), lambda: Q.direct_pixel_expectation(view, geo, table, cam, PIXEL_N))
    rp = _frame_params(mcpt, view)
    scene.trace_stats()
    got = direct_frame(scene, rp, illum=Q.ILLUM)
    st = scene.trace_stats()
    assert same(direct_frame(scene, rp, illum=Q.ILLUM, lean=1), got)
    assert st["paths"] == PIXEL_N and st["shades"] == PIXEL_N and st["rays"] == 2 * PIXEL_N
    Q.check_direct(_where("direct pixel", layout), name, got.reshape(-1, 3), PIXEL_SPP, E, var)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", Q.AO_PIXEL, ids=Q.ao_id)
def test_ao_frame_against_the_closed_form(mcpt, oracle_mod, world, expected, case, layout):
    """N = 2^18: resolves 5 sqrt((1 - p) / (N p)), the plates (p 0.068 .. 0.083) 3.6 .. 3.2 %, the lid at radius 1.25 from
    under it, with the pixel form's literal bias 0.01 (p = 1 - 1 / 1.26^2 = 0.370) 1.3 %."""
    name, radius = case
    scene, geo, _ = world(name, layout)
    view = Q.View(name)
    _, cam = camera(oracle_mod, view)
    p_occ = expected(("ao pixel",) + case, lambda: Q.ao_pixel_expectation(view, geo, cam, radius, PIXEL_N))
    if name == "lid":
        assert abs(p_occ - (1.0 - 1.0 / 1.26 ** 2)) < 1e-6
    rp = _frame_params(mcpt, view)
    scene.trace_stats()
    got = ao_frame(scene, rp, radius=radius)
    st = scene.trace_stats()
    assert same(ao_frame(scene, rp, radius=radius, lean=1), got)
    assert st["paths"] == PIXEL_N and st["shades"] == PIXEL_N and st["rays"] == 2 * PIXEL_N
    Q.check_ao(_where("ao pixel", layout), Q.ao_id(case), got, PIXEL_SPP, p_occ)

"""The restatements of the ambient-occlusion and the direct-lighting queries
(tests/_ao_ref.py, tests/_direct_ref.py) against closed-form radiometry
(tests/_query_radiometry.py): Lambert's form factor as the probability that an occlusion
ray is stopped, the cap 1 - (h / (radius + bias))^2 under a plane within reach, and the
float64 moments of the area-sampling estimator Ka illum cx cy A_tot / (pi r^2).  The kernels
equal the restatements bit for bit (test_gpu_ao.py, test_gpu_direct.py); this module asks
whether the shared expressions compute the right quantity, and
tests/test_gpu_query_radiometry.py asks the kernels the same with 16 times the samples.

Point forms: 256 copies of the case's point, stream ids 0 .. 255, 1024 samples each,
N = 2^18, the library's default seed.  Pixel forms: the narrow camera of
test_radiometry_cpu.py, 32 x 32 px, 64 spp, N = 2^16.  Asserted (check_ao, check_direct):
the z-test with Z_MAX = 5, the dispersion of the per-stream values within
1 +- 5 sqrt(2 / (R - 1)) and their lag-1 autocorrelation within 5 / sqrt R; sigma is the closed
form's own.  The first part checks the closed forms against the textbook and themselves.

The uniforms of a stream depend on the ids, the sample range and the seed alone, so the
module draws each set once (`shared_draws`).  Each test prints its figures
(profiles/radiometry/z_table.md is made of them).
"""
import math

import numpy as np
import pytest

import _ao_ref as A
import _direct_ref as D
import _query_radiometry as Q
import _radiometry as R
from _query_radiometry import query_radiometry_scenes  # noqa: F401  (a fixture)
from _radiometry import radiometry_scenes  # noqa: F401  (a fixture)
from test_radiometry_cpu import camera

STREAMS, SPP = 256, 1024
N = STREAMS * SPP
PIXEL_SPP = 64
PIXEL_N = R.PX * R.PX * PIXEL_SPP


# ---- the reference against itself and the textbook ------------------------------

def _two(quad):
    q = np.asarray(quad, np.float64)
    return [q[[0, 1, 2]], q[[0, 2, 3]]]


def _lights(tris, ng, kai=(1.0, 1.0, 1.0)):
    return [(t, ng, np.asarray(kai, np.float64)) for t in tris]


@pytest.mark.parametrize("a,b,h", [(1.0, 1.0, 1.0), (4.0, 2.5, 7.0), (2.0, 3.0, 1.5)])
def test_first_moment_of_a_rectangle_from_under_its_corner(a, b, h):
    rect = np.array([(0, h, 0), (a, h, 0), (a, h, b), (0, h, b)], np.float64)
    want = R.rect_corner_form_factor(a, b, h)
    e, var = Q.direct_moments((0, 0, 0), (0, 1, 0), _lights(_two(rect), (0, -1, 0), (1.0, 0.5, 0.0)))
    assert np.abs(e - want * np.array([1.0, 0.5, 0.0])).max() < 1e-9
    assert var[0] > 0 and abs(var[1] - 0.25 * var[0]) < 1e-12 and var[2] == 0
    # the same rectangle and point in a tilted frame
    e1, e2, e3 = R._frame(R.N3)
    tilted = np.array([v[0] * e1 + v[2] * e2 + v[1] * e3 + 5.0 for v in rect])
    et, vt = Q.direct_moments((5, 5, 5), e3, _lights(_two(tilted), e3, (1.0, 0.5, 0.0)))
    assert np.abs(et - e).max() < 1e-9 and np.abs(vt - var).max() < 1e-9


def test_moments_are_additive_over_a_split_light():
    x, n = np.array(R.plate_aim("P3")), np.array(R.N3)
    light = np.asarray(R.LIGHT, np.float64)
    m01, m23 = (light[0] + light[1]) / 2, (light[2] + light[3]) / 2
    whole = Q.direct_moments(x, n, _lights(_two(light), (0, -1, 0)))
    split = Q.direct_moments(x, n, _lights(_two([light[0], m01, m23, light[3]]) + _two([m01, light[1], light[2], m23]),
                                           (0, -1, 0)))
    for a, b in zip(whole, split):
        assert np.abs(a - b).max() < 1e-9 * np.abs(a).max()
    assert abs(whole[0][0] - R.polygon_form_factor(x, n, light)) < 1e-9
    # a hole that is the second half leaves the first
    half = Q.direct_moments(x, n, _lights(_two(light), (0, -1, 0)), minus=[[m01, light[1], light[2], m23]])
    first = Q.direct_moments(x, n, _lights(_two([light[0], m01, m23, light[3]]), (0, -1, 0)))
    assert np.abs(half[0] - first[0]).max() < 1e-9
    # (the variance is not the half light's: the samples still spread over the whole area)
    assert half[1][0] > first[1][0]


def test_a_closed_box_of_uniform_radiance_gives_ka_illum():
    """Six emitting faces around a point: E = Ka illum exactly.  The floor and the walls' parts below
    the point's horizon radiate nothing towards it (max(n.d, 0) = 0), so the sum runs over the ceiling
    and the walls above the horizon; the normal is the box's axis, the point off its centre."""
    X, Y, Z, y0 = 3.0, 5.0, 4.0, 1.0
    x = np.array([0.5, y0, -0.75])
    faces = [([(-X, Y, -Z), (X, Y, -Z), (X, Y, Z), (-X, Y, Z)], (0, -1, 0)),
             ([(-X, y0, -Z), (X, y0, -Z), (X, Y, -Z), (-X, Y, -Z)], (0, 0, 1)),
             ([(-X, y0, Z), (X, y0, Z), (X, Y, Z), (-X, Y, Z)], (0, 0, -1)),
             ([(-X, y0, -Z), (-X, y0, Z), (-X, Y, Z), (-X, Y, -Z)], (1, 0, 0)),
             ([(X, y0, -Z), (X, y0, Z), (X, Y, Z), (X, Y, -Z)], (-1, 0, 0))]
    kai = np.array([0.75, 0.5, 0.25]) * 2.0
    lights = [light for quad, ng in faces for light in _lights(_two(quad), ng, kai)]
    e, var = Q.direct_moments(x, (0, 1, 0), lights)
    assert np.abs(e - kai).max() < 1e-9
    assert (var > 0).all()


@pytest.mark.parametrize("h,radius,bias", [(1.0, 2.0, 1 / 64), (1.0, 1.0, 1 / 64), (0.5, 3.0, 0.25), (2.0, 2.5, 0.0)])
def test_ao_cap_probability_is_a_discs_form_factor(h, radius, bias):
    """the plane within reach is a disc of radius rho = sqrt((radius + bias)^2 - h^2) over the point:
    sin^2 theta = rho^2 / (rho^2 + h^2), between a 64-gon's form factor and its inscribed disc's"""
    rho = math.sqrt((radius + bias) ** 2 - h * h)
    p = Q.ao_cap_probability(h, radius, bias)
    assert abs(p - rho * rho / (rho * rho + h * h)) < 1e-12
    k = np.arange(64) * (2.0 * math.pi / 64)
    for axis in ((0.0, 1.0, 0.0), R.N3):
        e1, e2, e3 = R._frame(axis)
        x = np.array([0.3, -0.2, 0.9])
        gon = [x + h * e3 + rho * (math.cos(t) * e1 + math.sin(t) * e2) for t in k]
        got = R.polygon_form_factor(x, e3, gon)
        inner = rho * math.cos(math.pi / 64)
        assert inner * inner / (inner * inner + h * h) < got < p
    assert Q.ao_cap_probability(1.0, 0.96875, 1 / 64) == 0.0 and Q.ao_cap_probability(1.0, 1.0, 0.0) == 0.0
    assert abs(Q.ao_cap_probability(1.0, 2.0, 1 / 64) - 0.753861) < 5e-7
    assert abs(Q.ao_cap_probability(1.0, 1.25, 1 / 64) - 0.375705) < 5e-7
    assert abs(Q.ao_cap_probability(1.0, 1.0, 1 / 64) - 0.030533) < 5e-7


def test_the_closed_forms_refuse_what_they_do_not_cover():
    lid = np.asarray(Q.LID, np.float64)
    foot = np.array([1.25, 2.0, -0.5])
    assert Q.ao_cap_probability(1.0, 2.0, 1 / 64, foot, lid) > 0.75
    with pytest.raises(AssertionError, match="leaves the occluder"):
        Q.ao_cap_probability(1.0, 8.0, 1 / 64, foot, lid)
    with pytest.raises(AssertionError, match="leaves the occluder"):
        Q.ao_cap_probability(1.0, 2.0, 1 / 64, np.array([8.0, 2.0, -0.5]), lid)
    with pytest.raises(AssertionError, match="not in the occluder's plane"):
        Q.ao_cap_probability(1.0, 2.0, 1 / 64, foot + (0, 0.5, 0), lid)
    x = np.asarray(R.plate_aim("P8"), np.float64)
    light, blocker = np.asarray(R.LIGHT, np.float64), np.asarray(R.BLOCKER, np.float64)
    shadow = Q.shadow_on(x, blocker, light)
    assert np.abs(shadow[:, 1] - 8.0).max() < 1e-12
    with pytest.raises(AssertionError, match="not inside the light"):
        Q.shadow_on(x, blocker + (4.0, 0.0, 0.0), light)
    with pytest.raises(AssertionError, match="not inside an emitter"):
        Q.direct_moments(x, (0, 1, 0), _lights(_two(light), (0, -1, 0)), minus=[shadow + (3.0, 0.0, 0.0)])
    with pytest.raises(AssertionError, match="not inside an emitter"):
        Q.direct_moments(x, (0, 1, 0), _lights(_two(light), (0, -1, 0)), minus=[blocker])
    # two polygons side by side are disjoint, overlapping ones are not
    assert Q.solid_angles_disjoint(x, (0, 1, 0), light, np.asarray(Q.TRI_B, np.float64))
    assert not Q.solid_angles_disjoint(x, (0, 1, 0), light, blocker)


def test_the_cases_are_the_issues():
    assert Q.DIRECT_POINT == tuple(R.PLATES) + ("L2",)
    assert len(Q.AO_POINT) == 8 + 4 + 1 and len(Q.AO_PIXEL) == 6 and len(Q.DIRECT_PIXEL) == 5
    for _, radius, bias in Q.AO_POINT:
        assert bias == 0.0 or math.frexp(bias)[0] == 0.5           # a power of two
    c = np.cross(np.subtract(Q.TRI_B[1], Q.TRI_B[0]), np.subtract(Q.TRI_B[2], Q.TRI_B[0]))
    assert 0.5 * math.sqrt(float(c @ c)) == 2.0 and c[1] < 0      # area 2, facing down
    for name in Q.SCENES:
        assert R.off_edges(R.quad(*R.PLATES["P1"][:3]), Q.View(name).aim)


# ---- the restatements against the closed forms -----------------------------------

@pytest.fixture(scope="module", autouse=True)
def shared_draws():
    """_ao_ref.stream_draws is a pure function of its arguments and most of a case's cost here:
    each set of uniforms is drawn once for the module"""
    memo, draw = {}, A.stream_draws

    def cached(oracle, ids, spp, spp_offset=0, seed=A.SEED, ndraws=4):
        key = (np.asarray(ids, np.uint32).tobytes(), spp, spp_offset, seed, ndraws)
        if key not in memo:
            memo[key] = draw(oracle, ids, spp, spp_offset, seed, ndraws)
            memo[key].setflags(write=False)
        return memo[key]

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(A, "stream_draws", cached)
        mp.setattr(D, "stream_draws", cached)
        yield


@pytest.fixture(scope="module")
def world(oracle_mod, radiometry_scenes, query_radiometry_scenes):  # noqa: F811
    """scene name -> (oracle scene, its geometry, its light table), loaded once"""
    have = {}
    paths = dict(radiometry_scenes, **query_radiometry_scenes)

    def get(name):
        if name not in have:
            s = oracle_mod.Scene(paths[name])
            have[name] = (s, R.Geometry(s), D.light_table(s))
        return have[name]

    return get


def _copies(x, ns):
    return np.tile(x, (STREAMS, 1)), np.tile(ns, (STREAMS, 1)), np.arange(STREAMS, dtype=np.uint32)


@pytest.mark.parametrize("name", Q.DIRECT_POINT)
def test_direct_restatement_against_the_closed_form(oracle_mod, world, name):
    """N = 2^18 samples at the case's one point, illum 2, the default bias.  The z-test resolves a relative
    error of E of 5 (sigma / E) / sqrt N: 0.10 % at sigma / E = 0.10 (P5), 0.16 % at 0.16 (P1), 0.4 % at 0.42 (P8;
    L2's green and blue 0.39)."""
    oscene, geo, table = world(name)
    view = Q.View(name)
    x, ns = view.point(geo)
    E, var = Q.direct_expectation(view, geo, table, x, ns)
    p, nrm, ids = _copies(x, ns)
    out, rec, vis = D.point_reference(oracle_mod, oscene, table, p, nrm, ids, SPP, illum=Q.ILLUM)
    assert rec["valid"].all()                       # every sample forms a shadow ray
    assert vis.all() == (name != "P8")
    Q.check_direct("restatement point", name, out, SPP, E, var)


@pytest.mark.parametrize("case", Q.AO_POINT, ids=Q.ao_id)
def test_ao_restatement_against_the_closed_form(oracle_mod, world, case):
    """N = 2^18.  Resolves a relative error of p of 5 sqrt((1 - p) / (N p)): the plates (p 0.068 .. 0.183)
    3.6 .. 2.1 %, the lid at radius 2 (0.754) 0.6 %, 1.25 (0.376) 1.3 %, 1.0 (0.0305) 5.5 % -- where the rule
    without the bias term gives exactly 0 -- and P8's blocker alone (0.0112) 9.2 %.  The lid at radius
    0.96875 is a counting statement: radius + bias < h, nothing is occluded."""
    name, radius, bias = case
    oscene, geo, _ = world(name)
    view = Q.View(name)
    x, ns = view.point(geo)
    p_occ = Q.ao_probability(view, geo, x, ns, radius, bias)
    p, nrm, ids = _copies(x, ns)
    out, occ = A.point_reference(oracle_mod, oscene, p, nrm, ids, SPP, radius=radius, bias=bias)
    assert N - int(R.counts(out, SPP, 1.0).sum()) == int(occ.sum())
    Q.check_ao("restatement point", Q.ao_id(case), out, SPP, p_occ)


def _camera(oracle_mod, view):
    _, cam = camera(oracle_mod, view)
    return cam, dict(fov=view.fov, eye=tuple(float(v) for v in view.eye), direction=tuple(view.direction), up=view.up)


@pytest.mark.parametrize("name", Q.DIRECT_PIXEL)
def test_direct_pixel_restatement_against_the_closed_form(oracle_mod, world, name):
    """32 x 32 px, 64 spp, N = 2^16: resolves 5 (sigma / E) / sqrt N, 0.32 % at sigma / E = 0.16 (P1) to 0.8 % at
    0.42 (P8).  P6 is seen from behind (the flip), P7 shades with a normal off the face's."""
    oscene, geo, table = world(name)
    view = Q.View(name)
    cam, kw = _camera(oracle_mod, view)
    E, var = Q.direct_pixel_expectation(view, geo, table, cam, PIXEL_N)
    rec, fr = D.pixel_samples(oracle_mod, oscene, table, R.PX, R.PX, PIXEL_SPP, **kw)
    assert fr["hit"].all() and rec["valid"].all()
    assert fr["flip"].all() == (name == "P6") and fr["flip"].any() == (name == "P6")
    out, _ = D.pixel_reference(oracle_mod, oscene, table, rec, illum=Q.ILLUM)
    Q.check_direct("restatement pixel", name, out.reshape(-1, 3), PIXEL_SPP, E, var)


@pytest.mark.parametrize("case", Q.AO_PIXEL, ids=Q.ao_id)
def test_ao_pixel_restatement_against_the_closed_form(oracle_mod, world, case):
    """32 x 32 px, 64 spp, N = 2^16: resolves 5 sqrt((1 - p) / (N p)), the plates (p 0.068 .. 0.083) 7.2 .. 6.5 %,
    the lid at radius 1.25 with the pixel form's literal bias 0.01 (p = 1 - 1 / 1.26^2 = 0.370) 2.5 %."""
    name, radius = case
    oscene, geo, _ = world(name)
    view = Q.View(name)
    cam, kw = _camera(oracle_mod, view)
    p_occ = Q.ao_pixel_expectation(view, geo, cam, radius, PIXEL_N)
    if name == "lid":
        assert abs(p_occ - (1.0 - 1.0 / 1.26 ** 2)) < 1e-6
    fr = A.frame(oracle_mod, oscene, R.PX, R.PX, PIXEL_SPP, **kw)
    assert fr["hit"].all()
    out, occ = A.pixel_reference(oracle_mod, oscene, fr, radius)
    assert PIXEL_N - int(R.counts(out, PIXEL_SPP, 1.0).sum()) == int(occ.sum())
    Q.check_ao("restatement pixel", Q.ao_id(case), out, PIXEL_SPP, p_occ)

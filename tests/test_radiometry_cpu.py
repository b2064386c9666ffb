"""The samplers and the path loop of the CPU oracle against closed-form radiometry
(tests/_radiometry.py): Lambert's point-to-polygon form factor under the
cosine-weighted hemisphere and its tangent frame, Schlick's transmission and
total internal reflection under the Fresnel sampler, the Phong lobe at normal
incidence, a closed emitting box.  The GPU kernels equal this oracle bit for bit
(every other module); this one asks whether the shared expressions compute the
right quantity.  tests/test_gpu_radiometry.py asks the kernels the same.

Every case is rendered through a camera of 0.25 degrees and 32 x 32 pixels three
units before its aim point, 256 samples a pixel: N = 2^18 samples of one Bernoulli
variable.  Its probability p is the mean of the closed form over the pixel
centres' hit points (guarded: the mean over the corners of the jitter's support
differs by less than 0.05 sigma / sqrt N).  Asserted: the counts are integers and
equal in the channels, |k - N p| <= 5 sqrt(N p (1 - p)), the dispersion and the lag-1
autocorrelation of the per-pixel counts (check_counts), and where every sample has
one exact value (the dome, the pane's totals, total internal reflection) at most
16 in 2^20 differ.  At N = 2^18 the test resolves a relative error of
5 sqrt((1 - p) / (N p)): 3.6 % at p = 0.07, 1 % at p = 0.5.

Seeds are the library default (CVMCTracer mode) and the frame seeds 0 .. 255
(QuinEngine mode), fixed before the first run.  Each test prints its figures
(profiles/radiometry/z_table.md is made of them).
"""
import math

import numpy as np
import pytest

import _radiometry as R
from _radiometry import radiometry_scenes  # noqa: F401  (a fixture)

SPP = 256
N = R.PX * R.PX * SPP
FRAMES = 256
QE_CASES = ("P1", "P3", "pane-front60-fkd0", "pane-back70-fkd0")


# ---- the reference against itself and the textbook ------------------------------

@pytest.mark.parametrize("a,b,h", [(1.0, 1.0, 1.0), (4.0, 2.5, 7.0), (0.3, 9.0, 0.7)])
def test_form_factor_of_a_rectangle_from_under_its_corner(a, b, h):
    rect = [(0, h, 0), (a, h, 0), (a, h, b), (0, h, b)]
    assert abs(R.polygon_form_factor((0, 0, 0), (0, 1, 0), rect) - R.rect_corner_form_factor(a, b, h)) < 1e-12
    # the same rectangle and point in a tilted frame
    e1, e2, e3 = R._frame(R.N3)
    tilted = [v[0] * e1 + v[2] * e2 + v[1] * e3 + 5.0 for v in np.asarray(rect, np.float64)]
    assert abs(R.polygon_form_factor((5, 5, 5), e3, tilted) - R.rect_corner_form_factor(a, b, h)) < 1e-12


def test_form_factor_is_additive_and_tends_to_one():
    x, n = np.array(R.plate_aim("P3")), np.array(R.N3)
    light = np.asarray(R.LIGHT, np.float64)
    whole = R.polygon_form_factor(x, n, light)
    m01, m23 = (light[0] + light[1]) / 2, (light[2] + light[3]) / 2
    halves = R.polygon_form_factor(x, n, [light[0], m01, m23, light[3]]) + R.polygon_form_factor(x, n, [m01, light[1], light[2], m23])
    tris = R.polygon_form_factor(x, n, light[[0, 1, 2]]) + R.polygon_form_factor(x, n, light[[0, 2, 3]])
    assert abs(whole - halves) < 1e-12 and abs(whole - tris) < 1e-12 and 0.01 < whole < 0.5
    huge = [(-1e6, 1, -1e6), (1e6, 1, -1e6), (1e6, 1, 1e6), (-1e6, 1, 1e6)]
    assert abs(R.polygon_form_factor((0, 0, 0), (0, 1, 0), huge) - 1.0) < 1e-5
    with pytest.raises(AssertionError):
        R.polygon_form_factor((0, 0, 0), (0, 1, 0), [(0, -1, 0), (1, 1, 0), (0, 1, 1)])


@pytest.mark.parametrize("ns1", [2.0, 11.0, 1001.0])
@pytest.mark.parametrize("radius,h", [(2.0, 4.0), (0.25, 4.0), (5.0, 1.0)])
def test_phong_lobe_probability_of_a_disc_like_polygon(ns1, radius, h):
    """between the inscribed and the circumscribed disc's 1 - cos(theta / 2)^ns1; and in any frame"""
    k = np.arange(64) * (2.0 * math.pi / 64)
    for axis in ((0.0, 1.0, 0.0), R.N3):
        e1, e2, e3 = R._frame(axis)
        x = np.array([0.3, -0.2, 0.9])
        gon = [x + h * e3 + radius * (math.cos(t) * e1 + math.sin(t) * e2) for t in k]
        got = R.phong_lobe_probability(x, e3, gon, ns1)
        lo = 1.0 - math.cos(0.5 * math.atan(radius * math.cos(math.pi / 64) / h)) ** ns1
        hi = 1.0 - math.cos(0.5 * math.atan(radius / h)) ** ns1
        assert lo <= got <= hi and (hi == 1.0 or lo < got < hi), (lo, got, hi)     # (ns1 1001 saturates the widest disc)


def test_fresnel_T():
    assert R.fresnel_T(-1.0, 0.9, 1.5, False) == 0.9 and R.fresnel_T(0.0, 0.9, 1.5, False) == 0.0
    assert abs(R.fresnel_T(-0.5, 0.9, 1.5, False) - 0.9 * (1 - 0.5 ** 5)) < 1e-15
    crit = math.degrees(math.asin(1 / 1.5))
    assert 41.0 < crit < 43.0
    assert R.fresnel_T(math.cos(math.radians(41)), 0.9, 1.5, True) > 0.5
    assert R.fresnel_T(math.cos(math.radians(43)), 0.9, 1.5, True) == 0.0
    assert R.fresnel_T(math.cos(math.radians(43)), 0.9, 1.5, False) > 0.5


def test_the_cases_are_the_issues():
    assert len(R.CASES) == 8 + 2 * 9 + 3 + 2 and len(R.CASE) == len(R.CASES)
    for c in R.CASES:
        assert c.value in (0.25, 0.5, 0.75, 1.0, 2.0), c
        assert abs(np.cross(c.direction, c.up)).max() > 0.1, c       # up is not parallel to the direction


# ---- the oracle against the closed forms ------------------------------------------

@pytest.fixture(scope="module")
def world(oracle_mod, radiometry_scenes):  # noqa: F811
    """scene name -> (oracle scene, its geometry), loaded once"""
    have = {}

    def get(name):
        if name not in have:
            s = oracle_mod.Scene(radiometry_scenes[name])
            have[name] = (s, R.Geometry(s))
        return have[name]

    return get


def camera(oracle_mod, case, qe=False, **kw):
    """the narrow camera's oracle parameters and its basis for _radiometry.pixel_rays"""
    p = oracle_mod.RenderParams(width=R.PX, height=R.PX, fov=case.fov, eye=tuple(case.eye), direction=tuple(case.direction),
                                up=case.up, threads=16, mode=oracle_mod.MODE_QE if qe else oracle_mod.MODE_CV, **kw)
    P = p.to_c()
    cam = dict(eye=[float(x) for x in P.eye], fwd=list(P.fwd), up=list(P.up), right=list(P.right))
    if qe:
        cam["qe_proj"] = (float(P.proj11), float(P.proj22))
    else:
        cam["cv_tan"] = float(P.tan_half_fov)
    return p, cam


def check_counts(case, img, spp, p, where):
    """The assertions on one image (H, W, 3) of means over spp samples, each pixel (or ray) a stream
    of its own: integer counts, the leak cap, the z-test, and over the streams' counts the dispersion
    (their variance over the binomial's spp p (1 - p), within 1 +- 5 sqrt(2 / (R - 1)) for R streams)
    and the lag-1 autocorrelation along the stream id (within 5 / sqrt R).  Prints the figures."""
    n = img.shape[0] * img.shape[1] * spp
    cap = R.leak_cap(n)
    if case.kind == "pane":
        cells, other = (R.counts(img[..., ch], spp, case.value) for ch in case.channels)
        assert not img[..., 1].any()
        leak = n - int(cells.sum() + other.sum())
        assert 0 <= leak <= cap, (case, leak)
        if case.name in R.TIR:                                # a counting statement, not a statistical one
            assert p == 1.0 and other.sum() == 0
            print("RADIOMETRY|%s|%s|p=1|k=%d|N=%d|z=-|leak=%d" % (where, case.name, cells.sum(), n, leak))
            return
    else:
        ks = [R.counts(img[..., ch], spp, case.value) for ch in range(3)]
        assert np.array_equal(ks[0], ks[1]) and np.array_equal(ks[0], ks[2])
        cells, leak = ks[0], 0
        if case.kind == "exact":
            leak = n - int(cells.sum())
            assert p == 1.0 and 0 <= leak <= cap, (case, leak)
            print("RADIOMETRY|%s|%s|p=1|k=%d|N=%d|z=-|leak=%d" % (where, case.name, cells.sum(), n, leak))
            return
    k, streams = int(cells.sum()), cells.size
    z, disp, rho = R.zscore(k, n, p), R.dispersion(cells, spp, p), R.lag1(cells.ravel())
    print("RADIOMETRY|%s|%s|p=%.6f|k=%d|N=%d|z=%+.2f|leak=%d|resolves=%.2f%%|dispersion=%.3f|lag1=%+.3f" %
          (where, case.name, p, k, n, z, leak, 100 * R.resolvable(n, min(p, 1 - p)), disp, rho))
    assert abs(z) <= R.Z_MAX, (case, where, z)
    assert abs(disp - 1.0) <= 5.0 * math.sqrt(2.0 / (streams - 1)), (case, where, disp)
    assert abs(rho) <= 5.0 / math.sqrt(streams), (case, where, rho)


@pytest.mark.parametrize("depth", [1, 7])
@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_oracle_against_the_closed_form(oracle_mod, world, case, depth):
    """Depth 1 meets the emitter in the final intersect, depth 7 inside the loop; one expectation.
    N = 2^18: the z-test resolves a relative error of p of 5 sqrt((1 - p) / (N p)): the plates (p 0.068..0.091) 3.1..3.6 %,
    P2 (0.183) 2.1 %; the pane's reflected share at 0..41 degrees (0.100) 2.9 %, 60 (0.128) 2.6 %, 80 (0.447) 1.1 %,
    88 (0.854; of the transmitted share) 2.4 %; Phong Ns 10 (0.304) 1.5 %, Ns 1000 (0.458) 1.1 %.  Back 43 and 70
    degrees and the dome are counting statements: at most 4 of the 2^18 samples may differ."""
    scene, geo = world(case.scene)
    params, cam = camera(oracle_mod, case, spp=SPP, max_depth=depth, illum=case.illum, fresnel_kd=case.fresnel_kd)
    p = R.render_expectation(case, geo, cam, N)
    img, cnt = scene.render(params)
    assert cnt["paths"] == N
    if case.kind == "exact":
        assert cnt["rays"] == 2 * cnt["paths"]
    check_counts(case, img, SPP, p, "oracle depth %d" % depth)


@pytest.mark.parametrize("name", QE_CASES)
def test_oracle_quinengine_mode_against_the_closed_form(oracle_mod, world, name):
    """QuinEngine mode: TEA-16 seeds, its own camera and path loop; 1 spp, depth 5, frame seeds
    0 .. 255, each frame gamma-encoded, so a hit is a non-zero channel.  N = 2^18: resolves P1 and P3
    (p 0.083) to 3.2 %, the pane at 60 degrees (0.128) to 2.6 %; back 70 degrees counts"""
    case = R.CASE[name]
    scene, geo = world(case.scene)
    hits = np.zeros((R.PX, R.PX, 3), np.float32)
    for seed in range(FRAMES):
        params, cam = camera(oracle_mod, case, qe=True, spp=1, max_depth=5, illum=1.0, fresnel_kd=0, seed=seed)
        img, cnt = scene.render(params)
        assert cnt["paths"] == R.PX * R.PX
        hits += (img > 0)
    assert FRAMES * R.PX * R.PX >= 1 << 18
    p = R.render_expectation(case, geo, cam, N)
    check_counts(QeView(case), hits / np.float32(FRAMES), FRAMES, p, "oracle quinengine")


class QeView:
    """a case whose samples count 1 each (hits counted from gamma-encoded frames)"""

    def __init__(self, case):
        self.name, self.kind, self.channels, self.value = case.name, case.kind, case.channels, 1.0

    def __repr__(self):
        return self.name

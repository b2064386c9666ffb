"""Closed-form radiometry for the ambient-occlusion and the direct-lighting queries: a
float64 reference (plain numpy, nothing of the product or the oracle in it), two more
scenes and the cases asked of both query kinds.

The bit-for-bit modules (test_gpu_ao.py, test_gpu_direct.py) compare the kernels with
restatements written from them, one float operation at a time: a wrong constant in
g = cx cy A_tot / (pi r^2), a triangle warp that is not uniform, a cdf that is not weighted by
area, a Ka of the wrong light, a missing |.| on the emitter's cosine, a radius measured from
the wrong origin or correlated draws would pass them all.  Here both kinds are set up on
tests/_radiometry.py's plates so that what they return has a closed form:

* ambient occlusion is a Bernoulli variable: a cosine-hemisphere ray meets a polygon with
  probability F, Lambert's point-to-polygon form factor (`R.polygon_form_factor`); under a
  large plane at height h, within `radius` of an origin `bias` along the ray, with
  probability 1 - (h / (radius + bias))^2 (`ao_cap_probability`).  The unoccluded samples
  are counted in integers, so `check_ao` is `check_counts`' three assertions.
* a direct-lighting sample is Ka illum g(y) if y is visible, y uniform over the emitters'
  area A_tot.  With f(y) = max(n.d, 0) |ng.d| / (pi r^2) its mean is
  E_c = sum_l Ka_l,c illum int_l f dA (the form factor again), its second moment
  A_tot sum_l (Ka_l,c illum)^2 int_l f^2 dA; both by tensor Gauss-Legendre on the
  Duffy-mapped triangles (`direct_moments`).  The z-test's sigma is the reference's own.

Scenes: the plates P1 .. P8; `L2`, plate P1 under the quad light and a small red triangle
(unequal areas, distances and Ka: red sees F_A + F_B, green and blue F_A); `lid`, plate P1
one unit under a black quad of 16 x 16 (an occluder and no emitter).

The triangle test is strict, so a ray through a triangulation diagonal misses both
triangles: at most 16 rays in 2^20 do.  For ambient occlusion that moves at most 64 of 2^22
samples against a sigma of about 560 counts; for the direct queries it touches only P8's
blocker, a relative 1e-5 of the value.  Both are below what the tests resolve and get no
allowance of their own.

`query_radiometry_scenes` is a session fixture, imported by the modules that use it.
"""
import math

import numpy as np
import pytest

import _radiometry as R

f32 = np.float32
DEFAULT_BIAS = float(f32(0.01))          # what bias = 0 means to both query kinds, and the pixel forms' literal

# -------------------------------------------------------------------- closed forms

_GL = {k: np.polynomial.legendre.leggauss(k) for k in (48, 64)}


def _triangle_moments(x, n, tri, ng, nodes):
    """(int f dA, int f^2 dA) over one triangle, f(y) = max(n.d, 0) |ng.d| / (pi r^2): Duffy's map
    y = v0 + s ((1 - t) e1 + t e2), dA = 2 A s ds dt, Gauss-Legendre with `nodes` points each way"""
    gx, gw = _GL[nodes]
    s, w = 0.5 * (gx + 1.0), 0.5 * gw
    S, T = np.meshgrid(s, s, indexing="ij")
    W = w[:, None] * w[None, :] * S
    e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
    y = tri[0] + S[..., None] * ((1.0 - T)[..., None] * e1 + T[..., None] * e2)
    v = y - x
    r2 = (v * v).sum(axis=-1)
    d = v / np.sqrt(r2)[..., None]
    f = np.maximum(d @ n, 0.0) * np.abs(d @ ng) / (math.pi * r2)
    c = np.cross(e1, e2)
    a2 = math.sqrt(float(c @ c))
    return a2 * float((W * f).sum()), a2 * float((W * f * f).sum())


def _inside_triangle(tri, p, tol=1e-9):
    e1, e2, v = tri[1] - tri[0], tri[2] - tri[0], p - tri[0]
    c = np.cross(e1, e2)
    b, g = float(np.cross(v, e2) @ c) / float(c @ c), float(np.cross(e1, v) @ c) / float(c @ c)
    return b >= -tol and g >= -tol and b + g <= 1.0 + tol


def direct_moments(x, n, lights, minus=()):
    """Mean E (3,) and variance (3,) of one sample of the direct estimator at the point x with unit
    normal n.  lights: (triangle float64 (3, 3), geometric normal, Ka illum (3,)) per light triangle;
    minus: polygons in an emitter's plane, inside the emitter, whose integrals are subtracted (a
    blocker's central projection from x, `shadow_on`).  Asserts that every first moment int f dA
    equals Lambert's form factor to 1e-9 and that 48 and 64 nodes agree to 1e-9 relative in both
    moments, so a badly converged sigma cannot loosen a test."""
    x, n = np.asarray(x, np.float64), R._unit(n)
    lights = [(np.asarray(t, np.float64), R._unit(g), np.asarray(k, np.float64)) for t, g, k in lights]
    area = 0.0
    for tri, _, _ in lights:
        c = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        area += 0.5 * math.sqrt(float(c @ c))
    holes = []                               # (fan triangle, the emitter's normal, its Ka illum)
    for poly in minus:
        poly = np.asarray(poly, np.float64)
        own = [(t, g, k) for t, g, k in lights if np.abs((poly - t[0]) @ g).max() < 1e-9]     # the lights in its plane
        assert own and all(any(_inside_triangle(t, p) for t, _, _ in own) for p in poly), \
            "direct_moments: a subtracted polygon is not inside an emitter in its plane"
        assert all(np.array_equal(own[0][2], k) for _, _, k in own)
        holes += [(poly[[0, i, i + 1]], own[0][1], own[0][2]) for i in range(1, len(poly) - 1)]
    out = {}
    for nodes in (48, 64):
        e, m2 = np.zeros(3), np.zeros(3)
        for sign, parts in ((1.0, lights), (-1.0, holes)):
            for tri, ng, kai in parts:
                i1, i2 = _triangle_moments(x, n, tri, ng, nodes)
                assert abs(i1 - R.polygon_form_factor(x, n, tri)) < 1e-9, (nodes, i1)
                e += sign * kai * i1
                m2 += sign * area * kai * kai * i2
        out[nodes] = (e, m2)
    for a, b in zip(out[48], out[64]):
        assert (np.abs(a - b) <= 1e-9 * np.abs(b)).all(), (a, b)
    e, m2 = out[64]
    return e, m2 - e * e


def shadow_on(x, blocker, light):
    """the blocker's central projection from x onto the plane of the convex polygon `light`; it
    stands for the blocker only where the blocker, seen from x, lies inside the light (asserted)"""
    x, light = np.asarray(x, np.float64), np.asarray(light, np.float64)
    blocker = np.asarray(blocker, np.float64)
    assert R.solid_angle_inside(x, blocker, light), "shadow_on: the blocker is not inside the light's solid angle"
    ng = np.cross(light[1] - light[0], light[2] - light[0])
    t = ((light[0] - x) @ ng) / ((blocker - x) @ ng)
    assert (t > 1.0).all()                   # between the point and the light
    return x + t[:, None] * (blocker - x)


def ao_cap_probability(h, radius, bias, foot=None, occluder=None):
    """Probability that a cosine-hemisphere ray from a surface point, its origin `bias` along its own
    direction and its reach t < radius from that origin (include/mcpt.h), meets a plane parallel to
    the surface at height h: the ray reaches it iff cos > h / (radius + bias), and
    P(cos > c) = 1 - c^2.  Holds while the disc of radius sqrt((radius + bias)^2 - h^2) about the
    point's foot on the plane lies inside the occluder: asserted against the convex polygon."""
    reach = radius + bias
    if reach <= h:
        return 0.0
    if occluder is not None:
        disc = math.sqrt(reach * reach - h * h)
        p = np.asarray(occluder, np.float64)
        foot = np.asarray(foot, np.float64)
        nrm = R._unit(np.cross(p[1] - p[0], p[2] - p[0]))
        assert abs(float((foot - p[0]) @ nrm)) < 1e-6, "ao_cap_probability: the foot is not in the occluder's plane"
        centre = p.mean(axis=0)
        for i in range(len(p)):
            a, b = p[i], p[(i + 1) % len(p)]
            inward = np.cross(nrm, b - a)
            inward = R._unit(inward if float(inward @ (centre - a)) > 0 else -inward)
            assert float((foot - a) @ inward) > disc, "ao_cap_probability: the disc leaves the occluder"
    return max(0.0, 1.0 - (h / reach) ** 2)


def solid_angles_disjoint(x, n, a, b):
    """do the convex polygons a and b, both above the plane (x, n), cover disjoint solid angles seen
    from x?  Their gnomonic images on the plane at unit height are convex: a separating edge."""
    e1, e2, e3 = R._frame(n)

    def image(poly):
        r = np.asarray(poly, np.float64) - np.asarray(x, np.float64)
        assert (r @ e3 > 0).all()
        return np.stack([(r @ e1) / (r @ e3), (r @ e2) / (r @ e3)], axis=1)

    pa, pb = image(a), image(b)
    for p, q in ((pa, pb), (pb, pa)):
        for i in range(len(p)):
            e = p[(i + 1) % len(p)] - p[i]
            axis = np.array([-e[1], e[0]])
            sp, sq = (p - p[i]) @ axis, (q - p[i]) @ axis
            if sq.max() < sp.min() or sq.min() > sp.max():
                return True
    return False


# -------------------------------------------------------------------------- scenes

TRI_B = [(3, 5, -3), (5, 5, -3), (3, 5, -1)]                  # L2's second light: material red, area 2
LID = R.quad((1, 2, -1), (1, 0, 0), (0, 0, 1), 8.0)           # one unit above plate P1
LID_EYE_DISTANCE = 0.5                                        # the lid's camera stands between plate and lid


def _plate_p1(name):
    c, U, V, n, recv, _ = R.PLATES["P1"]
    return R._Obj(name).polygon("plate", recv, R.quad(c, U, V), n)


def l2_obj():
    o = _plate_p1("L2").polygon("light", "glow", R.LIGHT, (0, -1, 0))
    return o.polygon("light2", "red", TRI_B, (0, -1, 0)).text()


def lid_obj():
    return _plate_p1("lid").polygon("lid", "black", LID, (0, -1, 0)).text()


OBJS = {"L2": l2_obj, "lid": lid_obj}
SCENES = tuple(OBJS)


@pytest.fixture(scope="session")
def query_radiometry_scenes(tmp_path_factory):
    """name -> .obj path"""
    paths = {}
    for name in SCENES:
        d = tmp_path_factory.mktemp("query_radiometry_" + name)
        (d / (name + ".obj")).write_text(OBJS[name]())
        (d / (name + ".mtl")).write_text(R.MTL)
        paths[name] = str(d / (name + ".obj"))
    return paths


# --------------------------------------------------------------------------- cases

ILLUM = 2.0
DIRECT_POINT = ("P1", "P2", "P3", "P4", "P5", "P6", "P7", "P8", "L2")
# (scene, radius, bias): radius 0 is unbounded, bias 0 the default 0.01; the stated ones are dyadic
AO_POINT = tuple((p, 0.0, 0.0) for p in R.PLATES) + (
    ("lid", 2.0, 1 / 64), ("lid", 1.25, 1 / 64), ("lid", 1.0, 1 / 64), ("lid", 0.96875, 1 / 64), ("P8", 6.5, 0.0))
DIRECT_PIXEL = ("P1", "P3", "P6", "P7", "P8")
AO_PIXEL = tuple((p, 0.0) for p in DIRECT_PIXEL) + (("lid", 1.25),)


def ao_id(case):
    return "-".join([case[0]] + ["r%g" % case[1]] * (case[1] != 0))


class View:
    """the fixed ray and the narrow camera of a scene: R.CASE's for a plate; plate P1's for L2; for
    the lid P1's from half a unit above the plate, under the lid"""

    def __init__(self, scene):
        plate = scene if scene in R.PLATES else "P1"
        c = R.CASE[plate]
        self.name, self.scene, self.plate = scene, scene, plate
        self.side = -1.0 if plate == "P6" else 1.0
        self.aim, self.direction, self.up, self.fov = c.aim, c.direction, c.up, c.fov
        self.eye = self.aim - (LID_EYE_DISTANCE if scene == "lid" else R.EYE_DISTANCE) * self.direction

    def ray(self):
        return self.eye.astype(f32), self.direction.astype(f32)

    def point(self, geo):
        """where the ray meets the plate and the point's unit normal, as the device takes them
        (float32) and as the closed forms do (the same numbers in float64)"""
        x = geo.plane_hit("plate", *self.ray()).astype(f32)
        ns = (geo.normal["plate"] * self.side).astype(f32)
        return x, ns

    def __repr__(self):
        return self.name


def lights_of(table, illum=ILLUM):
    """_direct_ref.light_table's (or Scene.lights() and the kd vertices') rows as direct_moments takes them"""
    return [(table["verts"][k].astype(np.float64), table["normals"][k].astype(np.float64),
             table["ka"][k].astype(np.float64) * illum) for k in range(table["kd_ids"].shape[0])]


def direct_expectation(view, geo, table, x, ns, illum=ILLUM):
    """(E (3,), variance (3,)) of one direct sample at x"""
    minus = [shadow_on(x, geo.poly["blocker"], geo.poly["light"])] if view.scene == "P8" else []
    if view.scene == "L2":                   # neither light hides the other
        a, b = geo.poly["light"], geo.poly["light2"]
        assert not R.solid_angle_inside(x, a, b) and not R.solid_angle_inside(x, b, a)
        assert solid_angles_disjoint(x, ns, a, b)
    return direct_moments(x, ns, lights_of(table, illum), minus)


def ao_probability(view, geo, x, ns, radius, bias):
    """the probability that one ambient-occlusion sample at x is occluded"""
    x, ns = np.asarray(x, np.float64), R._unit(ns)
    b = DEFAULT_BIAS if bias == 0 else bias
    if view.scene == "lid":
        lid = geo.poly["lid"]
        h = float((lid[0] - x) @ ns)
        return ao_cap_probability(h, radius, b, x + h * ns, lid)
    light = geo.poly["light"]
    if view.scene == "P8":
        blocker = geo.poly["blocker"]
        assert R.solid_angle_inside(x, blocker, light)
        if radius != 0:                      # only the blocker is within reach
            far = math.sqrt(float(((blocker - x) ** 2).sum(axis=1).max()))
            near = abs(float((light[0] - x) @ R._unit(np.cross(light[1] - light[0], light[2] - light[0]))))
            assert far + b < radius and radius + b < near, (far, near)
            return R.polygon_form_factor(x, ns, blocker)
    assert radius == 0
    return R.polygon_form_factor(x, ns, light)


def pixel_points(view, geo, cam, xs, ys):
    """where the narrow camera's rays through the raster positions meet the plate: (len(ys) len(xs), 3)"""
    return geo.plane_hit("plate", *R.pixel_rays(xs=xs, ys=ys, **cam)).reshape(-1, 3)


def _centres_and_corners(view, geo, cam):
    c = np.arange(R.PX, dtype=np.float64)
    e = np.arange(-1, R.PX + 1, dtype=np.float64)[[0, -1]]
    return pixel_points(view, geo, cam, c, c), pixel_points(view, geo, cam, e, e)


def ao_pixel_expectation(view, geo, cam, radius, n):
    """The mean of the closed form over the pixel centres' hit points, and R.render_expectation's
    guard: the mean over the corners of the jitter's support differs by < 0.05 sigma / sqrt(N)."""
    ns = geo.normal["plate"] * view.side
    centres, corners = _centres_and_corners(view, geo, cam)
    p = float(np.mean([ao_probability(view, geo, x, ns, radius, 0.0) for x in centres]))
    pc = float(np.mean([ao_probability(view, geo, x, ns, radius, 0.0) for x in corners]))
    if 0.0 < p < 1.0:
        assert abs(pc - p) < 0.05 * math.sqrt(p * (1.0 - p) / n), (view, p, pc)
    return p


def direct_pixel_expectation(view, geo, table, cam, n, illum=ILLUM):
    """(E, variance) of one sample of the pixel form: the moments' means over the pixel centres' hit
    points; the guard as above, with this estimator's own sigma"""
    ns = geo.normal["plate"] * view.side
    centres, corners = _centres_and_corners(view, geo, cam)
    mo = [direct_expectation(view, geo, table, x, ns, illum) for x in centres]
    e = np.mean([m[0] for m in mo], axis=0)
    m2 = np.mean([m[1] + m[0] * m[0] for m in mo], axis=0)
    var = m2 - e * e
    ec = np.mean([direct_expectation(view, geo, table, x, ns, illum)[0] for x in corners], axis=0)
    assert (np.abs(ec - e) < 0.05 * np.sqrt(var / n)).all(), (view, e, ec)
    return e, var


# -------------------------------------------------------------------------- checks

def check_ao(where, name, ao, spp, p_occ):
    """The assertions on R per-stream means `ao` of spp ambient-occlusion samples each (a sample is 1
    if unoccluded): check_counts' three, with its constants -- |z| <= Z_MAX of the occluded count k
    against N p_occ, the dispersion of the per-stream counts within 1 +- 5 sqrt(2 / (R - 1)), their
    lag-1 autocorrelation within 5 / sqrt R.  p_occ 0 or 1 is a counting statement.  Prints the figures."""
    open_ = R.counts(np.asarray(ao).ravel(), spp, 1.0)
    streams = open_.size
    n = streams * spp
    k = n - int(open_.sum())
    if p_occ == 0.0 or p_occ == 1.0:
        print("RADIOMETRY|%s|%s|p=%d|k=%d|N=%d|z=-|dispersion=-|lag1=-|resolves=-" % (where, name, p_occ, k, n))
        if p_occ == 0.0:
            assert k == 0, (where, name, k)
        else:
            assert 0 <= n - k <= R.leak_cap(n), (where, name, k)
        return
    z, disp, rho = R.zscore(k, n, p_occ), R.dispersion(open_, spp, p_occ), R.lag1(open_)
    print("RADIOMETRY|%s|%s|p=%.6f|k=%d|N=%d|z=%+.2f|dispersion=%.3f|lag1=%+.3f|resolves=%.2f%%" %
          (where, name, p_occ, k, n, z, disp, rho, 100 * R.Z_MAX * math.sqrt(p_occ * (1.0 - p_occ) / n) / p_occ))
    assert abs(z) <= R.Z_MAX, (where, name, z)
    assert abs(disp - 1.0) <= 5.0 * math.sqrt(2.0 / (streams - 1)), (where, name, disp)
    assert abs(rho) <= 5.0 / math.sqrt(streams), (where, name, rho)


def check_direct(where, name, out, spp, E, var):
    """The assertions on R per-stream means `out` (R, 3) of spp direct-lighting samples each, per
    channel of positive variance: |mean - E| <= Z_MAX sqrt(var / N), the streams' variance times spp
    over var within 1 +- 5 sqrt(2 / (R - 1)), their lag-1 autocorrelation within 5 / sqrt R.  A channel
    of expectation 0 is exactly 0.  Prints the figures."""
    out = np.asarray(out, np.float64).reshape(-1, 3)
    streams = out.shape[0]
    n = streams * spp
    fails, seen = [], {}
    for c in range(3):
        if E[c] == 0.0:
            print("RADIOMETRY|%s|%s %s|E=0|mean=%g|N=%d|z=-|dispersion=-|lag1=-|resolves=-" %
                  (where, name, "rgb"[c], out[:, c].max(), n))
            assert not out[:, c].any(), (where, name, c)
            continue
        assert var[c] > 0.0, (where, name, c)
        key = (E[c], var[c], out[:, c].tobytes())
        if key in seen:                      # a channel that repeats an earlier one, bit for bit: the same figures
            print("RADIOMETRY|%s|%s %s|as %s" % (where, name, "rgb"[c], "rgb"[seen[key]]))
            continue
        seen[key] = c
        mean = float(out[:, c].mean())
        z = (mean - E[c]) / math.sqrt(var[c] / n)
        disp = float(np.var(out[:, c], ddof=1)) * spp / var[c]
        rho = R.lag1(out[:, c])
        print("RADIOMETRY|%s|%s %s|E=%.7f|mean=%.7f|N=%d|z=%+.2f|dispersion=%.3f|lag1=%+.3f|resolves=%.3f%%" %
              (where, name, "rgb"[c], E[c], mean, n, z, disp, rho, 100 * R.Z_MAX * math.sqrt(var[c] / n) / E[c]))
        if abs(z) > R.Z_MAX:
            fails.append(("z", c, z))
        if abs(disp - 1.0) > 5.0 * math.sqrt(2.0 / (streams - 1)):
            fails.append(("dispersion", c, disp))
        if abs(rho) > 5.0 / math.sqrt(streams):
            fails.append(("lag1", c, rho))
    assert not fails, (where, name, fails)

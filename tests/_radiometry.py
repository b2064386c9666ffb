"""Closed-form radiometry for the samplers and the path loop: a float64 reference
(plain numpy, nothing of the product or the oracle in it) and the scenes it is
asked about.

Every other GPU test asks whether the kernel equals the oracle bit for bit; the
two share every float expression, so a wrong tangent frame, a hemisphere that is
not cosine-distributed, a Fresnel exponent off by one, a Phong lobe with the wrong
exponent or correlated seeds would pass them all.  Here a path of one bounce is
set up so that what it returns is a Bernoulli variable whose probability has a
closed form:

* plate   a diffuse 2 x 2 quad under a polygonal emitter: the cosine-weighted
          hemisphere sample reaches the emitter with probability F, Lambert's
          point-to-polygon form factor (`polygon_form_factor`)
* pane    a glass quad between a red and a blue emitting wall: the sample is
          transmitted with probability T = Tr (1 - (1 - |cos|)^5), never beyond the
          critical angle from inside (`fresnel_T`)
* phong   a glossy floor under a square emitter, normal incidence: the reflected
          ray has polar angle 2T, cos T = u^(1/(Ns+1)), uniform azimuth
          (`phong_lobe_probability`)
* dome    a closed emitting box over a diffuse floor: every sample returns
          exactly Kd Ka illum

All material values are dyadic, so with a power of two of samples every mean is
an exact multiple of the sample value and hit counts come back as integers
(`counts`).  The triangle test is strict (beta > 0, gamma > 0, beta + gamma < 1, as
in the reference), so a ray through an edge shared by two triangles misses both:
every aim point sits off every triangulation edge (asserted when the cases are
made), and what still leaks on secondary rays is capped (`leak_cap`).

All text is built from the literal coordinates below by Python float arithmetic
and %.6f; the closed forms take the float32 vertices and normals read back from
the loaded model (`Geometry`), not the text.  `radiometry_scenes` is a session
fixture, imported by the modules that use it.
"""
import math

import numpy as np
import pytest

# ------------------------------------------------------------------ closed forms


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def polygon_form_factor(x, n, poly):
    """Lambert's edge sum: the form factor of a planar polygon seen from the point x of a
    surface with unit normal n, F = |sum_i gamma_i n . (v_i x v_i+1) / |v_i x v_i+1|| / 2 pi with
    v_i the corners as seen from x and gamma_i the angle between v_i and v_i+1.  The polygon must
    lie above the plane (x, n): it is not clipped."""
    x, n = np.asarray(x, np.float64), _unit(n)
    r = np.asarray(poly, np.float64) - x
    assert (r @ n >= 0.0).all(), "polygon_form_factor: the polygon reaches below the horizon"
    r = _unit(r)
    total = 0.0
    for i in range(len(r)):
        a, b = r[i], r[(i + 1) % len(r)]
        c = np.cross(a, b)
        s = math.sqrt(float(c @ c))
        total += math.atan2(s, float(a @ b)) * float(n @ c) / s
    return abs(total) / (2.0 * math.pi)


def fresnel_T(cos_i, Tr, Ni, leaving):
    """probability that the sample is transmitted: Tr (1 - (1 - |cos|)^5); nothing leaves the
    denser side beyond the critical angle, 1 - (1 - cos^2) Ni^2 < 0"""
    c = abs(float(cos_i))
    if leaving and 1.0 - (1.0 - c * c) * Ni * Ni < 0.0:
        return 0.0
    return Tr * (1.0 - (1.0 - c) ** 5)


_GL_X, _GL_W = np.polynomial.legendre.leggauss(64)


def _frame(axis):
    axis = _unit(axis)
    k = int(np.argmin(np.abs(axis)))
    e1 = _unit(np.cross(axis, np.eye(3)[k]))
    return e1, np.cross(axis, e1), axis


def phong_lobe_probability(x, axis, poly, ns1):
    """Probability that the Phong sample of a ray arriving along -axis (normal incidence; axis the
    unit normal) reaches the convex polygon that surrounds the axis: the reflected direction has
    polar angle 2T with cos T = u^(1/ns1) and uniform azimuth, so
    P = (1/2 pi) closed-integral [1 - cos(theta_max(phi) / 2)^ns1] d phi, theta_max(phi) where the
    azimuth half-plane meets the polygon's boundary; Gauss-Legendre, 64 nodes per edge span."""
    e1, e2, e3 = _frame(axis)
    r = np.asarray(poly, np.float64) - np.asarray(x, np.float64)
    q = np.stack([r @ e1, r @ e2, r @ e3], axis=1)
    assert (q[:, 2] > 0.0).all()
    phi = np.arctan2(q[:, 1], q[:, 0])
    total, turn = 0.0, 0.0
    for i in range(len(q)):
        a, d = q[i], q[(i + 1) % len(q)] - q[i]
        dphi = (phi[(i + 1) % len(q)] - phi[i] + math.pi) % (2.0 * math.pi) - math.pi
        turn += dphi
        f = phi[i] + 0.5 * dphi * (_GL_X + 1.0)
        s = (a[0] * np.sin(f) - a[1] * np.cos(f)) / (d[1] * np.cos(f) - d[0] * np.sin(f))
        assert (s > -1e-9).all() and (s < 1.0 + 1e-9).all()
        p = a[None, :] + s[:, None] * d[None, :]
        theta = np.arctan2(np.hypot(p[:, 0], p[:, 1]), p[:, 2])
        total += 0.5 * abs(dphi) * float((_GL_W * (1.0 - np.cos(0.5 * theta) ** ns1)).sum())
    assert abs(abs(turn) - 2.0 * math.pi) < 1e-9, "phong_lobe_probability: the polygon does not surround the axis"
    return total / (2.0 * math.pi)


def rect_corner_form_factor(a, b, h):
    """the textbook case: a rectangle a x b parallel to the surface at height h, one corner over the point"""
    p, q = math.sqrt(a * a + h * h), math.sqrt(b * b + h * h)
    return (a / p * math.atan(b / p) + b / q * math.atan(a / q)) / (2.0 * math.pi)


def solid_angle_inside(x, inner, outer):
    """is every corner of the polygon `inner`, seen from x, strictly inside the convex polygon `outer`?"""
    x = np.asarray(x, np.float64)
    o = np.asarray(outer, np.float64) - x
    planes = [np.cross(o[i], o[(i + 1) % len(o)]) for i in range(len(o))]
    centre = o.mean(axis=0)
    for v in np.asarray(inner, np.float64) - x:
        for pl in planes:
            if float(pl @ v) * float(pl @ centre) <= 0.0:
                return False
    return True


# ------------------------------------------------------------------------- numbers

Z_MAX = 5.0                     # |k - N p| <= 5 sqrt(N p (1 - p)); not a tuning knob


def leak_cap(n):
    """samples that may differ from the exact value where every sample has one: 16 per 2^20"""
    return (16 * n) >> 20


def zscore(k, n, p):
    return (k - n * p) / math.sqrt(n * p * (1.0 - p))


def resolvable(n, p):
    """the relative error of p that the z-test resolves with n samples"""
    return Z_MAX * math.sqrt((1.0 - p) / (n * p))


def counts(mean, spp, value):
    """per-ray or per-pixel means of spp samples, each 0 or `value` -> the number of samples that
    were `value`; asserts that it is an integer in [0, spp]"""
    k = np.asarray(mean, np.float64) * float(spp) / float(value)
    assert np.array_equal(k, np.rint(k)), "a mean is no whole multiple of the sample value"
    assert (k >= 0).all() and (k <= spp).all()
    return k.astype(np.int64)


def dispersion(k, spp, p):
    """variance of the per-stream counts over the binomial's, spp p (1 - p)"""
    return float(np.var(np.asarray(k, np.float64), ddof=1)) / (spp * p * (1.0 - p))


def lag1(k):
    """lag-1 autocorrelation of the per-stream counts over the stream id"""
    d = np.asarray(k, np.float64) - np.mean(k)
    return float((d[1:] * d[:-1]).sum() / (d * d).sum())


# -------------------------------------------------------------------------- scenes

MTL = ("newmtl recv\nKd 0.5 0.5 0.5\nKa 0 0 0\n"
       "newmtl recv75\nKd 0.75 0.75 0.75\nKa 0 0 0\n"
       "newmtl glow\nKd 0.5 0.5 0.5\nKa 1 1 1\n"
       "newmtl glow50\nKd 0.5 0.5 0.5\nKa 0.5 0.5 0.5\n"
       "newmtl black\nKd 0 0 0\nKa 0 0 0\n"
       "newmtl glass\nKd 0.5 0.5 0.5\nKa 0 0 0\nTr 0.9\nNi 1.5\n"
       "newmtl red\nKd 0.5 0.5 0.5\nKa 1 0 0\n"
       "newmtl blue\nKd 0.5 0.5 0.5\nKa 0 0 1\n"
       "newmtl phong10\nKd 0.25 0.25 0.25\nKa 0 0 0\nKs 0.5 0.5 0.5\nNs 10\n"
       "newmtl phong1000\nKd 0.25 0.25 0.25\nKa 0 0 0\nKs 0.5 0.5 0.5\nNs 1000\n")
KD = {"recv": 0.5, "recv75": 0.75, "glass": 0.5}
KA = {"glow": 1.0, "glow50": 0.5, "red": 1.0, "blue": 1.0}
KS = 0.5
GLASS_TR, GLASS_NI = 0.9, 1.5

C0 = (1.0, 1.0, -1.0)
LIGHT = [(-2, 8, -4), (2, 8, -4), (2, 8, 0), (-2, 8, 0)]
AIM_UV = (0.25, 0.5)
FOV, PX = 0.25, 32                                           # the narrow camera: degrees, pixels a side
EYE_DISTANCE = 3.0
N3 = (3 / 13, 12 / 13, 4 / 13)
U3, V3 = (0.8, 0.0, -0.6), (-36 / 65, 25 / 65, -48 / 65)
S401 = math.sqrt(401.0)


def _lin(c, *terms):
    return tuple(c[a] + sum(s * v[a] for s, v in terms) for a in range(3))


def quad(c, U, V, hu=1.0, hv=None):
    """corners c -+ hu U -+ hv V; the fan's diagonal runs from the first to the third"""
    hv = hu if hv is None else hv
    return [_lin(c, (su * hu, U), (sv * hv, V)) for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))]


def _mirror(p, c, n):
    d = sum((p[a] - c[a]) * n[a] for a in range(3))
    return tuple(p[a] - 2.0 * d * n[a] for a in range(3))


class _Obj:
    """OBJ text, one group and one face line per polygon, one normal per polygon"""

    def __init__(self, name):
        self.v, self.vn, self.f = ["mtllib %s.mtl" % name], [], []
        self.nv = self.nn = 0

    def polygon(self, group, material, corners, normal):
        self.v += ["v %.6f %.6f %.6f" % tuple(float(x) + 0.0 for x in c) for c in corners]
        self.vn.append("vn %.6f %.6f %.6f" % tuple(float(x) + 0.0 for x in normal))
        self.nn += 1
        self.f += ["g " + group, "usemtl " + material,
                   "f " + " ".join("%d//%d" % (self.nv + 1 + i, self.nn) for i in range(len(corners)))]
        self.nv += len(corners)
        return self

    def text(self):
        return "\n".join(self.v + self.vn + self.f) + "\n"


# name -> (centre, U, V, shading normal, receiver material, light material)
PLATES = {
    "P1": (C0, (1, 0, 0), (0, 0, 1), (0, 1, 0), "recv", "glow"),                   # the n.y - 1 pole branch
    "P2": ((1.0, 12.0, -1.0), (1, 0, 0), (0, 0, 1), (0, -1, 0), "recv", "glow"),   # n.y + 1; the light's back
    "P3": (C0, U3, V3, N3, "recv75", "glow50"),                                    # a general normal
    "P4": (C0, (0, 0, 1), (20 / S401, -1 / S401, 0), (1 / S401, 20 / S401, 0), "recv", "glow"),   # large invlen
    "P5": (C0, (0, 1, 0), (-0.8, 0, 0.6), (0.6, 0, 0.8), "recv", "glow"),          # n.y = 0
    "P6": (C0, U3, V3, N3, "recv", "glow"),                                        # P3 from behind: the flip
    "P7": (C0, (1, 0, 0), (0, 0, 1), N3, "recv", "glow"),                          # shading normal off the face's
    "P8": (C0, (1, 0, 0), (0, 0, 1), (0, 1, 0), "recv", "glow"),                   # P1 and a black blocker
}
BLOCKER = [(0, 6, -2), (1, 6, -2), (1, 6, -1), (0, 6, -1)]
PANE = [(-4, 0, 0), (4, 0, 0), (4, 8, 0), (-4, 8, 0)]
PANE_AIM = (1.0, 2.0, 0.0)
WALL = 1000.0
PHONG_C = (1.0, 0.0, -1.0)
DOME = (6.0, 8.0, 6.0)                                       # x in -6..6, y in 0..8, z in -6..6


def plate_aim(name):
    c, U, V = PLATES[name][:3]
    return _lin(c, (AIM_UV[0], U), (AIM_UV[1], V))


def plate_light(name):
    c, U, V, n = PLATES[name][:4]
    if name == "P5":                     # the quad light is below this plate's horizon: one in its own frame
        return quad(_lin(c, (7.0, n), (1.0, U)), U, V, 2.0)
    if name == "P6":                     # the quad light mirrored through the plate's plane
        return [_mirror(p, c, n) for p in LIGHT]
    return LIGHT


def plate_obj(name):
    c, U, V, n, recv, glow = PLATES[name]
    o = _Obj(name).polygon("plate", recv, quad(c, U, V), n)
    o.polygon("light", glow, plate_light(name), (0, -1, 0))
    if name == "P8":
        o.polygon("blocker", "black", BLOCKER, (0, -1, 0))
    return o.text()


def pane_obj():
    o = _Obj("pane").polygon("pane", "glass", PANE, (0, 0, 1))
    for group, z, nz in (("red", 10.0, -1), ("blue", -10.0, 1)):
        o.polygon(group, group, [(-WALL, -WALL, z), (WALL, -WALL, z), (WALL, WALL, z), (-WALL, WALL, z)], (0, 0, nz))
    return o.text()


def phong_floor_aim():
    return _lin(PHONG_C, (AIM_UV[0], (1, 0, 0)), (AIM_UV[1], (0, 0, 1)))


def phong_obj(name):
    """phong10 / phong1000: a floor and a square light centred over the aim point at height 4;
    phong10t: plate P3's quad with the light built in its frame"""
    if name == "phong10t":
        c, U, V, n = PLATES["P3"][:4]
        o = _Obj(name).polygon("plate", "phong10", quad(c, U, V), n)
        return o.polygon("light", "glow", quad(_lin(plate_aim("P3"), (4.0, n)), U, V, 2.0), n).text()
    half = 2.0 if name == "phong10" else 0.25
    o = _Obj(name).polygon("plate", name, quad(PHONG_C, (1, 0, 0), (0, 0, 1)), (0, 1, 0))
    return o.polygon("light", "glow", quad(_lin(phong_floor_aim(), (4.0, (0, 1, 0))), (1, 0, 0), (0, 0, 1), half),
                     (0, -1, 0)).text()


def dome_obj():
    X, Y, Z = DOME
    o = _Obj("dome").polygon("plate", "recv", [(-X, 0, -Z), (X, 0, -Z), (X, 0, Z), (-X, 0, Z)], (0, 1, 0))
    o.polygon("ceiling", "glow", [(-X, Y, -Z), (X, Y, -Z), (X, Y, Z), (-X, Y, Z)], (0, -1, 0))
    o.polygon("back", "glow", [(-X, 0, -Z), (X, 0, -Z), (X, Y, -Z), (-X, Y, -Z)], (0, 0, 1))
    o.polygon("front", "glow", [(-X, 0, Z), (X, 0, Z), (X, Y, Z), (-X, Y, Z)], (0, 0, -1))
    o.polygon("left", "glow", [(-X, 0, -Z), (-X, 0, Z), (-X, Y, Z), (-X, Y, -Z)], (1, 0, 0))
    o.polygon("right", "glow", [(X, 0, -Z), (X, 0, Z), (X, Y, Z), (X, Y, -Z)], (-1, 0, 0))
    return o.text()


OBJS = dict({p: (lambda p=p: plate_obj(p)) for p in PLATES}, pane=pane_obj, dome=dome_obj,
            **{p: (lambda p=p: phong_obj(p)) for p in ("phong10", "phong1000", "phong10t")})
SCENES = tuple(OBJS)
# where the whole arrangement is in view at the default field of view (the renders against the oracle)
OVERVIEW = dict({p: dict(eye=(1.0, 12.0, 10.0), direction=(0.0, -0.7, -1.0)) for p in SCENES},
                P2=dict(eye=(1.0, 4.0, 10.0), direction=(0.0, 0.55, -1.0)),           # from below
                P5=dict(eye=(14.1, 3.0, -0.2), direction=(-11.0, -2.0, 2.0)),         # from the side the plate faces
                P6=dict(eye=(-5.25, -13.0, 1.67), direction=(0.44, 1.06, -0.41)),     # the plates' view, mirrored
                pane=dict(eye=(9.0, 4.0, 6.0), direction=(-1.0, 0.0, -0.8)),
                dome=dict(eye=(0.0, 4.0, 5.5), direction=(0.0, -0.3, -1.0)))


@pytest.fixture(scope="session")
def radiometry_scenes(tmp_path_factory):
    """name -> .obj path"""
    paths = {}
    for name in SCENES:
        d = tmp_path_factory.mktemp("radiometry_" + name)
        (d / (name + ".obj")).write_text(OBJS[name]())
        (d / (name + ".mtl")).write_text(MTL)
        paths[name] = str(d / (name + ".obj"))
    return paths


class Geometry:
    """what the closed forms take from a loaded model (an oracle.Scene): each group's polygon in
    float64 from the float32 vertices, in the fan's order, and its float32 shading normal"""

    def __init__(self, oscene):
        v, t, nrm = oscene.vertices(), oscene.triangles(), oscene.normals()
        self.poly, self.normal = {}, {}
        for name, tris in oscene.groups().items():
            if len(tris) == 0:
                continue
            idx = list(t[tris[0], 0:3]) + [t[k, 2] for k in tris[1:]]
            self.poly[name] = v[idx].astype(np.float64)
            self.normal[name] = _unit(nrm[t[tris[0], 6]].astype(np.float64))

    def plane_hit(self, group, o, d):
        """where the rays o + t d meet the plane of the group's polygon (float64)"""
        p = self.poly[group]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        t = ((p[0] - o) @ n) / (d @ n)
        return o + np.asarray(t)[..., None] * d


def off_edges(poly, x, margin=0.05):
    """is x at least `margin` from every border and both diagonals of the quad?"""
    p = np.asarray(poly, np.float64)
    x = np.asarray(x, np.float64)
    lines = [(p[i], p[(i + 1) % 4]) for i in range(4)] + [(p[0], p[2]), (p[1], p[3])]
    for a, b in lines:
        e = _unit(b - a)
        r = x - a
        if math.sqrt(max(float(r @ r) - float(r @ e) ** 2, 0.0)) < margin:
            return False
    return True


# --------------------------------------------------------------------------- cases

class Case:
    """One fixed ray into one scene.  kind "count": the samples are `value` with probability
    p(geometry, hit point), 0 otherwise, equal in all three channels.  kind "pane": `value` in the
    reflected wall's channel with probability p (= 1 - T), in the other wall's otherwise.
    kind "exact": every sample is `value` (leak cap)."""

    def __init__(self, name, scene, kind, aim, direction, up, prob, value, illum=2.0, fresnel_kd=1, channels=None,
                 fov=FOV):
        self.name, self.scene, self.kind = name, scene, kind
        self.fov = fov                             # of the narrow camera (degrees)
        self.aim = np.asarray(aim, np.float64)
        self.direction = _unit(direction)
        self.up, self.prob, self.value, self.illum, self.fresnel_kd = up, prob, value, illum, fresnel_kd
        self.channels = channels                   # pane: (reflected wall's channel, the other's)
        self.eye = self.aim - EYE_DISTANCE * self.direction

    def ray(self):
        """the query's ray as the device takes it: float32 origin and unit direction"""
        return self.eye.astype(np.float32), self.direction.astype(np.float32)

    def p_at(self, geo, o, d):
        """the closed form at the points where rays (o, d) meet the plate; -> array of p"""
        x = geo.plane_hit("pane" if self.kind == "pane" else "plate", o, d)
        d = np.broadcast_to(_unit(d), x.shape)
        return np.array([self.prob(geo, xi, di) for xi, di in zip(x.reshape(-1, 3), d.reshape(-1, 3))])

    def __repr__(self):
        return self.name


def _plate_case(name):
    c, U, V, n, recv, glow = PLATES[name]
    side = -1.0 if name == "P6" else 1.0
    face = _unit(np.cross(U, V))
    if float(face @ np.asarray(n, np.float64)) < 0:
        face = -face
    aim = plate_aim(name)
    assert off_edges(quad(c, U, V), aim)

    def prob(geo, x, d):
        ns = geo.normal["plate"] * side
        light = geo.poly["light"]
        if name == "P7":                # above the shading normal's horizon and the face's (asserted in F, and here)
            assert ((light - x) @ face > 0).all()
        f = polygon_form_factor(x, ns, light)
        if name == "P8":
            assert solid_angle_inside(x, geo.poly["blocker"], light)
            f -= polygon_form_factor(x, ns, geo.poly["blocker"])
        return f

    up = (0.0, 0.0, -1.0) if abs(face[1]) > 0.9 else (0.0, 1.0, 0.0)
    return Case(name, name, "count", aim, -side * face, up, prob, KD[recv] * KA[glow] * 2.0)


PANE_ANGLES = [("front", a) for a in (0, 30, 60, 80, 88)] + [("back", a) for a in (20, 41, 43, 70)]


def _pane_case(side, angle, fkd):
    a = math.radians(angle)
    sz = -1.0 if side == "front" else 1.0              # front: from z > 0 towards -z
    direction = (-math.sin(a), 0.0, sz * math.cos(a))
    assert off_edges(PANE, PANE_AIM)

    def prob(geo, x, d):
        cos_i = float(_unit(d) @ geo.normal["pane"])
        assert (cos_i > 0) == (side == "back")
        return 1.0 - fresnel_T(cos_i, GLASS_TR, GLASS_NI, leaving=cos_i > 0)

    value = (KD["glass"] if fkd else 1.0) * 1.0 * 2.0
    channels = (0, 2) if side == "front" else (2, 0)   # front: reflected to the red wall at z = +10
    return Case("pane-%s%d-fkd%d" % (side, angle, fkd), "pane", "pane", PANE_AIM, direction, (0.0, 1.0, 0.0), prob,
                value, fresnel_kd=fkd, channels=channels)


def _phong_case(name):
    ns1 = 1001.0 if name == "phong1000" else 11.0
    if name == "phong10t":
        c, U, V, n = PLATES["P3"][:4]
        aim, direction, up = plate_aim("P3"), tuple(-x for x in n), (0.0, 1.0, 0.0)
        assert off_edges(quad(c, U, V), aim)
    else:
        aim, direction, up = phong_floor_aim(), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0)
        assert off_edges(quad(PHONG_C, (1, 0, 0), (0, 0, 1)), aim)

    def prob(geo, x, d):
        return phong_lobe_probability(x, geo.normal["plate"], geo.poly["light"], ns1)

    # (the narrow lobe of Ns 1000 varies over the 0.25-degree camera's footprint by more than the
    # guard of render_expectation allows: a quarter of the field of view)
    return Case(name, name, "count", aim, direction, up, prob, KS * 1.0 * 2.0,
                fov=FOV / 4 if name == "phong1000" else FOV)


DOME_VIEWS = {"dome-down": ((1.5, 0.0, -3.5), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0)),
              "dome-oblique": ((-2.0, 0.0, 3.5), (-0.48, -0.6, 0.64), (0.0, 1.0, 0.0))}


def _dome_case(name):
    aim, direction, up = DOME_VIEWS[name]
    X, Y, Z = DOME
    assert off_edges([(-X, 0, -Z), (X, 0, -Z), (X, 0, Z), (-X, 0, Z)], aim)
    eye = np.asarray(aim) - EYE_DISTANCE * _unit(direction)
    assert (np.abs(eye) < np.array([X, Y, Z]) - 0.05).all() and eye[1] > 0.05
    return Case(name, "dome", "exact", aim, direction, up, lambda geo, x, d: 1.0, KD["recv"] * 1.0 * 2.0)


def _cases():
    out = [_plate_case(p) for p in PLATES]
    out += [_pane_case(s, a, fkd) for fkd in (0, 1) for s, a in PANE_ANGLES]
    out += [_phong_case(p) for p in ("phong10", "phong1000", "phong10t")]
    out += [_dome_case(v) for v in DOME_VIEWS]
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}
TIR = {"pane-back43-fkd0", "pane-back43-fkd1", "pane-back70-fkd0", "pane-back70-fkd1"}

# ----------------------------------------------------------- the narrow-fov camera


def pixel_rays(eye, fwd, up, right, xs, ys, cv_tan=None, qe_proj=None, w=PX, h=PX):
    """float64 rays through the raster positions (xs, ys) of the render's camera: CVMCTracer's
    (tan of half the field of view over the width) or QuinEngine's (the projection's two scales);
    the jitter of both is symmetric about the whole-numbered position, the pixel's centre here"""
    xs, ys = np.meshgrid(np.asarray(xs, np.float64), np.asarray(ys, np.float64))
    if cv_tan is not None:
        ix = (2.0 * xs / w - 1.0) * cv_tan
        iy = (1.0 * h / w - 2.0 * ys / w) * cv_tan
    else:
        ix = (2.0 * xs / w - 1.0) / qe_proj[0]
        iy = (1.0 - 2.0 * ys / h) / qe_proj[1]
    f, u, r = (np.asarray(a, np.float64) for a in (fwd, up, right))
    d = ix[..., None] * r + iy[..., None] * u + f
    return np.broadcast_to(np.asarray(eye, np.float64), d.shape), _unit(d)


def render_expectation(case, geo, cam, n):
    """The mean of the closed form over the pixel centres' hit points, and the guard: the same mean
    over the corners of the jitter's support (one pixel either way) differs by < 0.05 sigma / sqrt(N)."""
    c = np.arange(PX, dtype=np.float64)
    e = np.arange(-1, PX + 1, dtype=np.float64)
    p = float(case.p_at(geo, *pixel_rays(xs=c, ys=c, **cam)).mean())
    pc = float(case.p_at(geo, *pixel_rays(xs=e[[0, -1]], ys=e[[0, -1]], **cam)).mean())
    if 0.0 < p < 1.0:
        assert abs(pc - p) < 0.05 * math.sqrt(p * (1.0 - p) / n), (case, p, pc)
    return p

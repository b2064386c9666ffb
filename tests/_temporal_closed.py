"""Closed-form reprojection for the temporal accumulation (csrc/temporal.hip, DESIGN.md
section 17): a float64 reference (plain numpy, nothing of the product, the oracle or
tests/_temporal_ref.py in it), analytic worlds, and the checks both
tests/test_temporal_closed_cpu.py (on the numpy restatement) and
tests/test_gpu_temporal_closed.py (on the kernel) run.

The bit-for-bit module (test_gpu_temporal.py) compares the kernel with a restatement written
from it one float operation at a time: a pixel centre half a pixel off, hw where 1 belongs, Wf
for Hf, a left-handed basis, a missing near-plane term, a wrong power of sw, a cap one too
high or a normal test scaled by one coverage would pass it, because the restatement shares
them.  Here the camera is derived the textbook way instead:

* an orthonormal right-handed look-at basis (f = direction / |direction|, r = f x up / |.|,
  u = r x f) from the float32 inputs the product receives, a 4 x 4 view matrix;
* a perspective map to NDC: CVMCTracer mode has the horizontal half-angle fov / 2 and square
  pixels (sx = cot(fov / 2), sy = sx W / H), QuinEngine mode the vertical fov and the aspect
  W / H (sy = cot(fov / 2), sx = sy / (W / H): PerspectiveFovRH);
* NDC to pixels with the centres at integers: x = (ndc_x + 1) W / 2, y = (1 - ndc_y) H / 2.

`pixel_ray` and `project` are written as inverses of each other.  In QuinEngine mode a ray
starts on the near plane, at forward distance 1 from the eye, and the depth of a point is
its distance from there.

Worlds (`World*`): per ray a surface id, the hit distance and the unit normal, from the
ray / plane, ray / rectangle and ray / sphere formulas.  Feature buffers are made from them
with one coverage for the whole frame, rounded once to float32.

Coordinate history: hist_color_n = (qx, qy, surface id of q, N0), this frame's colour 0.
Bilinear interpolation of a function linear in the pixel coordinates is exact, so for a
pixel that used every tap offered to it out.xy (N0 + 1) / N0 is the kernel's own (bx, by),
and out.z (N0 + 1) / N0 the surface id its history came from.

The hinge world and why its plate moves.  The cameras of the disocclusion cases are one
unit and a fifth apart at 16 units from the wall.  A strip that one of them sees and the
other does not is as wide as the camera shift times the relative depth gap behind the
occluder; at a relative gap below sigma_z = 0.1 that is at most 0.12 units, a quarter of a
pixel of the largest frame, at any angle of the plate (and a plate seen from its other side
after the move is 3 x 1.2 / 16 = 0.23 units wide).  No static plate on the wall can therefore
give a pixel whose surface is absent from the 3 x 3 block it lands in while the depths
agree.  So the plate swings: the previous frame shows the wall alone (the plate lay in it),
the current frame the plate turned about its edge on the wall.  The plate's pixels near
that edge land on wall pixels less than sigma_z away in depth, and only the normal test
keeps the wall's history out of them.  At 70 degrees the plate is so foreshortened that
the 23 x 37 CV frame holds none of them and the 37 x 23 one a single one; turned further,
to 145 degrees (35 from the wall on its other side, cos 35 = 0.82 < 0.9), every frame
holds at least 12.  The static hinge (`hinge-static`) is kept for what it can show:
footprints that straddle the edge take history from their own surface only.

Tolerances: TOL_PX and TOL_VAR below are 8 times the restatement's worst error against this
reference over all reprojection and variance cases, measured on the CPU (DESIGN.md section 17
records them).  The kernel is bit-equal to the restatement; the margin is for changes of the
cases.
"""
import math
from collections import namedtuple

import numpy as np

f32, f64 = np.float32, np.float64
N0 = 7.0                                 # the coordinate history's length
MISS, BEHIND, REJECTED, BILINEAR, FALLBACK = 0, 1, 2, 3, 4       # _temporal_ref's classes, by value

# 8 x the restatement's worst error against this reference (see the module docstring)
TOL_PX = 1.4e-4                          # pixels; measured 1.73e-5 (QuinEngine mode, 64 x 48)
TOL_VAR = 1.7e-4                         # relative, out_var of the variance case; measured 2.10e-5
TOL_BLEND = 1e-5                         # relative: a handful of float32 roundings per frame

SIZES = [(37, 23), (23, 37), (64, 48)]   # (W, H)
MODES = ["cv", "qe"]

Result = namedtuple("Result", "out out_var cls offered used")


# ---- the camera ------------------------------------------------------------------------------

def camera(mode, W, H, eye=(0.0, 5.0, 17.0), direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov=None):
    """the look-at camera of one frame, from the float32 values the product receives"""
    e, d, u0 = (np.asarray(v, f32).astype(f64) for v in (eye, direction, up))
    fov = float(f32((60.0 if mode == "cv" else 45.0) if fov is None else fov))
    f = d / np.linalg.norm(d)
    r = np.cross(f, u0)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    rot = np.stack([r, u, -f])           # world -> view: x right, y up, the camera looks down -z
    view = np.eye(4)
    view[:3, :3] = rot
    view[:3, 3] = -rot @ e
    cot = 1.0 / math.tan(math.radians(fov) / 2.0)
    if mode == "cv":
        sx = cot
        sy = sx * W / H
    else:
        sy = cot
        sx = sy / (W / H)
    return dict(mode=mode, W=W, H=H, eye=e, view=view, sx=sx, sy=sy)


def _to_view(cam, P):
    return P @ cam["view"][:3, :3].T + cam["view"][:3, 3]


def pixel_ray(cam, x, y):
    """origin and unit direction of the ray through pixel coordinates (x, y), fractional too"""
    x, y = np.asarray(x, f64), np.asarray(y, f64)
    nx, ny = 2.0 * x / cam["W"] - 1.0, 1.0 - 2.0 * y / cam["H"]
    dv = np.stack([nx / cam["sx"], ny / cam["sy"], -np.ones_like(nx)], -1)     # on the plane 1 in front
    w = dv @ cam["view"][:3, :3]
    d = w / np.linalg.norm(w, axis=-1, keepdims=True)
    o = cam["eye"] + (w if cam["mode"] == "qe" else np.zeros_like(w))
    return o, d


def project(cam, P):
    """(bx, by, depth along the ray that reaches P, in front of the camera?)"""
    P = np.asarray(P, f64)
    pv = _to_view(cam, P)
    zc = -pv[..., 2]
    with np.errstate(all="ignore"):
        nx, ny = cam["sx"] * pv[..., 0] / zc, cam["sy"] * pv[..., 1] / zc
        bx, by = (nx + 1.0) * 0.5 * cam["W"], (1.0 - ny) * 0.5 * cam["H"]
        v = P - cam["eye"]
        o = cam["eye"] + (v / zc[..., None] if cam["mode"] == "qe" else np.zeros_like(v))
        depth = np.linalg.norm(P - o, axis=-1)
    return bx, by, depth, zc > 0.0


# ---- the worlds ------------------------------------------------------------------------------

def _unit(v):
    v = np.asarray(v, f64)
    return v / np.linalg.norm(v)


class WorldPlane:
    """one oblique infinite plane"""

    def __init__(self, point=(0.0, 5.0, 2.0), normal=(0.25, 0.15, 1.0)):
        self.p, self.n = np.asarray(point, f64), _unit(normal)

    def __call__(self, o, d):
        t = ((self.p - o) @ self.n) / (d @ self.n)
        n = np.broadcast_to(self.n, d.shape) * -np.sign(d @ self.n)[..., None]
        return np.zeros(t.shape, np.int64), t, n


class WorldShell:
    """a sphere seen from inside, its normals radial (towards the centre)"""

    def __init__(self, centre, radius=14.0):
        self.c, self.r = np.asarray(centre, f64), float(radius)

    def __call__(self, o, d):
        oc = o - self.c
        b = (oc * d).sum(-1)
        t = -b + np.sqrt(b * b - ((oc * oc).sum(-1) - self.r * self.r))
        P = o + d * t[..., None]
        return np.zeros(t.shape, np.int64), t, (self.c - P) / self.r


class WorldWallPlate:
    """the wall z = 1 (id 0) and a square plate of half-width 1.5 (id 1): centred at (0, 5, 9)
    and facing +z, or (hinge: degrees) with one vertical edge on the wall at x = hinge_x and
    turned that far out of it; plate=False: the wall alone"""

    def __init__(self, hinge=None, hinge_x=-1.5, plate=True):
        self.plate = plate
        if hinge is None:
            self.c, self.a = np.array([0.0, 5.0, 9.0]), np.array([1.0, 0.0, 0.0])
        else:
            phi = math.radians(hinge)
            self.a = np.array([math.cos(phi), 0.0, math.sin(phi)])
            self.c = np.array([hinge_x, 5.0, 1.0]) + 1.5 * self.a
        self.b = np.array([0.0, 1.0, 0.0])
        self.n = np.cross(self.a, self.b)
        self.half = 1.5

    def __call__(self, o, d):
        tw = (1.0 - o[..., 2]) / d[..., 2]
        nz = np.array([0.0, 0.0, 1.0])
        sid, t = np.zeros(tw.shape, np.int64), tw.copy()
        n = np.broadcast_to(nz, d.shape) * -np.sign(d[..., 2])[..., None]
        if self.plate:
            dn = d @ self.n
            with np.errstate(all="ignore"):
                tp = ((self.c - o) @ self.n) / dn
                q = o + d * tp[..., None] - self.c
                on = (np.abs(q @ self.a) <= self.half) & (np.abs(q @ self.b) <= self.half) & (tp > 0.0) & (tp < tw)
            sid[on] = 1
            t[on] = tp[on]
            n = np.where(on[..., None], self.n * -np.sign(dn)[..., None], n)
        return sid, t, n


def frame(cam, world):
    """what every pixel centre of cam sees: sid, t, n, the point P (float64)"""
    ys, xs = np.mgrid[0:cam["H"], 0:cam["W"]]
    o, d = pixel_ray(cam, xs, ys)
    sid, t, n = world(o, d)
    assert np.isfinite(t).all() and (t > 0.0).all(), "a ray of this camera misses the world"
    return dict(sid=sid, t=t, n=n, P=o + d * t[..., None])


def features(fr, cov=1.0, n=None):
    """(albedo_cov, normal_depth) as csrc/aov.hip forms means of `cov` hits per sample"""
    H, W = fr["t"].shape
    ac = np.full((H, W, 4), cov, f32)
    nd = (np.concatenate([fr["n"] if n is None else n, fr["t"][..., None]], -1) * cov).astype(f32)
    return ac, nd


def coordinate_history(fr):
    H, W = fr["t"].shape
    ys, xs = np.mgrid[0:H, 0:W]
    return np.stack([xs, ys, fr["sid"], np.full((H, W), N0)], -1).astype(f32)


def landing(prev_cam, cur_fr):
    """where the current frame's points are in the previous frame: bx, by, the expected depth,
    inside (in front and in [0, W - 1] x [0, H - 1])"""
    bx, by, e, front = project(prev_cam, cur_fr["P"])
    with np.errstate(all="ignore"):
        inside = front & (bx >= 0.0) & (bx <= prev_cam["W"] - 1.0) & (by >= 0.0) & (by <= prev_cam["H"] - 1.0)
    return bx, by, e, inside


def _bufs(ac, nd, hist, hac, hnd, color=None, var=None, hist_var=None):
    H, W = ac.shape[:2]
    return dict(color=np.zeros((H, W, 3), f32) if color is None else color, var=var, albedo_cov=ac, normal_depth=nd,
                hist_color_n=hist, hist_var=hist_var, hist_albedo_cov=hac, hist_normal_depth=hnd)


def recovered(out):
    """(bx, by, surface id) a pixel's coordinate history was fetched at, from out of a frame of colour 0"""
    return out[..., :3].astype(f64) * ((N0 + 1.0) / N0)


def _all_full(res, mask):
    assert (res.cls[mask] == BILINEAR).all(), ("not bilinear", np.argwhere(mask & (res.cls != BILINEAR))[:5].tolist())
    assert (res.used[mask] == res.offered[mask]).all(), ("a tap offered was not used",
                                                         np.argwhere(mask & (res.used != res.offered))[:5].tolist())
    n = res.out[..., 3].astype(f64)
    assert (np.abs(n[mask] - (N0 + 1.0)) <= 2.0 * float(np.spacing(f32(N0 + 1.0)))).all(), "N != N0 + 1"


def _all_reset(res, mask, c=0.0):
    assert (res.out[..., 3][mask] == 1.0).all(), ("a history was found", np.argwhere(mask & (res.out[..., 3] != 1))[:5].tolist())
    assert (res.out[..., :3][mask] == f32(c)).all()
    assert np.isin(res.cls[mask], (MISS, BEHIND, REJECTED)).all()


# ---- the camera pairs ------------------------------------------------------------------------

def _fwd(direction):
    return tuple(float(v) for v in _unit(np.asarray(direction, f32).astype(f64)))


def pairs(mode):
    """name: (cur, prev) camera keywords: between them every degree of freedom moves"""
    qe = mode == "qe"
    dolly_dir = (0.05, -0.1, -1.0)
    step = 1.5 * np.asarray(_fwd(dolly_dir))
    return {
        "all": (dict(eye=(0.7, 5.3, 16.0), direction=(0.12, -0.2, -1.0), up=(0.15, 1.0, 0.05), fov=45.0 if qe else 50.0),
                dict(eye=(0.0, 5.0, 17.0), direction=(0.0, -0.1, -1.0), up=(-0.1, 1.0, 0.0), fov=40.0 if qe else 45.0)),
        # a pure dolly along fwd
        "dolly": (dict(eye=tuple(float(v) for v in np.array([0.0, 5.0, 17.0]) + step), direction=dolly_dir),
                  dict(eye=(0.0, 5.0, 17.0), direction=dolly_dir)),
        # a direction of length 3, an up that is not at right angles to it
        "long": (dict(eye=(0.5, 5.5, 16.5), direction=(0.3, -0.45, -2.95), up=(0.3, 1.0, -0.4)),
                 dict(eye=(0.0, 5.0, 17.0), direction=(0.0, 0.0, -3.0), up=(0.0, 1.0, 0.5))),
    }


DISOCCLUSION = (dict(eye=(1.2, 5.2, 17.0), direction=(0.03, -0.02, -1.0), up=(0.05, 1.0, 0.0)), dict())
RENDER_CAMERAS = {"default": dict(), "second": dict(eye=(1.0, 7.0, 16.0), direction=(0.15, -0.25, -1.0), up=(0.1, 1.0, 0.0))}
RENDER_SPP = 64


# ---- reprojection ------------------------------------------------------------------------

def check_reprojection(run, mode, W, H, cur_kw, prev_kw, tol=TOL_PX):
    """plane world, coordinate history: every pixel that lands inside the previous frame is
    bilinear with every tap offered, N = N0 + 1, and fetched its history at project(prev, P)"""
    cur, prev = camera(mode, W, H, **cur_kw), camera(mode, W, H, **prev_kw)
    world = WorldPlane()
    cf, pf = frame(cur, world), frame(prev, world)
    bx, by, _, inside = landing(prev, cf)
    frac = lambda a: a - np.floor(a)     # noqa: E731
    generic = inside & (frac(bx) >= 0.1) & (frac(bx) <= 0.9) & (frac(by) >= 0.1) & (frac(by) <= 0.9)
    assert inside.sum() >= W * H / 2 and generic.sum() >= 100, (int(inside.sum()), int(generic.sum()))
    res = run(mode, W, H, cur_kw, prev_kw, _bufs(*features(cf), coordinate_history(pf), *features(pf)))
    rec = recovered(res.out)
    err = np.maximum(np.abs(rec[..., 0] - bx), np.abs(rec[..., 1] - by))[inside]
    fig = dict(inside=int(inside.sum()), generic=int(generic.sum()), worst_px=float(err.max()))
    print("reprojection", mode, W, H, fig)
    _all_full(res, inside)
    assert err.max() <= tol, fig
    return fig


# ---- the depth term ----------------------------------------------------------------------

SHELL_SIGMA = {"cv": 2e-6, "qe": 2e-3}


def check_depth_term(run, mode, W=37, H=23):
    """shell world about the previous eye: CV mode's previous depths are exactly the radius,
    QuinEngine's the distance from the near plane.  Within sigma_z every inside pixel keeps
    all its taps; with the history's depths scaled by 1 +- 3 sigma_z none finds a history."""
    cur_kw, prev_kw = pairs(mode)["all"]
    cur, prev = camera(mode, W, H, **cur_kw), camera(mode, W, H, **prev_kw)
    world = WorldShell(prev["eye"])
    cf, pf = frame(cur, world), frame(prev, world)
    if mode == "cv":
        assert np.abs(pf["t"] - 14.0).max() < 1e-12
    else:
        assert 12.5 < pf["t"].min() < pf["t"].max() <= 13.0 and np.ptp(pf["t"]) > 0.05     # the near plane: about 1 in 13
    _, _, _, inside = landing(prev, cf)
    assert inside.sum() >= W * H / 2
    sz = SHELL_SIGMA[mode]
    ac, nd = features(cf)
    hac, hnd = features(pf)
    hist = coordinate_history(pf)
    _all_full(run(mode, W, H, cur_kw, prev_kw, _bufs(ac, nd, hist, hac, hnd), sigma_z=sz), inside)
    for s in (1.0 + 3.0 * sz, 1.0 - 3.0 * sz):
        off = hnd.copy()
        off[..., 3] = (pf["t"] * s).astype(f32)
        _all_reset(run(mode, W, H, cur_kw, prev_kw, _bufs(ac, nd, hist, hac, off), sigma_z=sz), inside)
    return dict(inside=int(inside.sum()))


# ---- the normal test under fractional coverages ---------------------------------------------

def _turned(n, cosine):
    """the unit normals n turned by acos(cosine) about an axis at right angles to them"""
    axis = np.cross(n, np.array([0.0, 1.0, 0.0]))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    return n * cosine + np.cross(axis, n) * math.sqrt(1.0 - cosine * cosine)


def check_normal_test(run, mode, thr, W=16, H=16, tol=TOL_PX):
    """plane world, this frame at coverage 0.5, the history at 0.75 (normal and depth both):
    a history normal turned by acos(thr + 0.01) keeps every tap, by acos(thr - 0.01) none;
    with unturned normals the coverages change nothing."""
    cur_kw, prev_kw = pairs(mode)["all"]
    cur, prev = camera(mode, W, H, **cur_kw), camera(mode, W, H, **prev_kw)
    world = WorldPlane()
    cf, pf = frame(cur, world), frame(prev, world)
    bx, by, _, inside = landing(prev, cf)
    assert inside.sum() >= W * H / 2
    hist = coordinate_history(pf)
    go = lambda a, b: run(mode, W, H, cur_kw, prev_kw, _bufs(*a, hist, *b), normal_threshold=thr)   # noqa: E731
    half = features(cf, 0.5)
    _all_full(go(half, features(pf, 0.75, _turned(pf["n"], thr + 0.01))), inside)
    _all_reset(go(half, features(pf, 0.75, _turned(pf["n"], thr - 0.01))), inside)
    res = go(half, features(pf, 0.75))
    _all_full(res, inside)
    rec = recovered(res.out)
    err = np.maximum(np.abs(rec[..., 0] - bx), np.abs(rec[..., 1] - by))[inside]
    assert err.max() <= tol, float(err.max())
    one = go(features(cf), features(pf))
    assert np.abs(recovered(one.out) - rec)[inside].max() <= tol
    return dict(inside=int(inside.sum()), worst_px=float(err.max()))


# ---- disocclusion --------------------------------------------------------------------------

def disocclusion_worlds():
    """name: (the current frame's world, the previous frame's, min must-reset, the share of
    undecided pixels allowed or None, min must-reset pixels only the normal can reject)"""
    return {"plate": (WorldWallPlate(), WorldWallPlate(), 8, 0.15, 0),
            "hinge": (WorldWallPlate(hinge=HINGE_DEGREES), WorldWallPlate(plate=False), 8, 0.15, 8),
            "hinge-static": (WorldWallPlate(hinge=HINGE_DEGREES), WorldWallPlate(hinge=HINGE_DEGREES), 0, None, 0)}


SIGMA_Z_DEFAULT = 0.1
# the sizes the caps on must-reset and undecided pixels hold at: at 23 x 37 a CV-mode pixel is 0.8
# units wide on the wall and the plate's 1.2-unit strip gives 6 must-reset pixels, not 8
CAPPED_SIZES = [(37, 23), (64, 48)]
HINGE_DEGREES = 145.0                    # 70 gives 0 to 14 normal-only pixels at these sizes, 110 4 to 36, 145 12 to 107


def classify_disocclusion(prev, cf, pf):
    """from surface ids alone: must_reuse, must_reset, undecided, and the must-reset pixels
    whose depth is within sigma_z of every footprint pixel's"""
    H, W = cf["sid"].shape
    bx, by, e, inside = landing(prev, cf)
    x0, y0 = np.floor(np.where(inside, bx, 0)).astype(int), np.floor(np.where(inside, by, 0)).astype(int)
    cx, cy = np.floor(np.where(inside, bx, 0) + 0.5).astype(int), np.floor(np.where(inside, by, 0) + 0.5).astype(int)
    fx, fy = bx - x0, by - y0
    away = lambda f: (f > 1e-3) & (f < 1.0 - 1e-3)   # noqa: E731
    same4 = np.ones((H, W), bool)
    none = np.ones((H, W), bool)
    close = np.ones((H, W), bool)
    taps = [(x0 + dx, y0 + dy, True) for dy in (0, 1) for dx in (0, 1)]
    taps += [(cx + dx, cy + dy, False) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    for qx, qy, bil in taps:
        ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
        jx, jy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
        same = pf["sid"][jy, jx] == cf["sid"]
        if bil:
            same4 &= ok & same           # (an inside pixel away from the integers is offered all four)
        none &= ~(ok & same)
        zq = pf["depth"][jy, jx]
        close &= ~ok | (np.abs(e - zq) < SIGMA_Z_DEFAULT * np.maximum(e, zq))
    must_reuse = inside & same4 & away(fx) & away(fy)
    must_reset = inside & none
    return dict(bx=bx, by=by, inside=inside, must_reuse=must_reuse, must_reset=must_reset,
                undecided=inside & ~must_reuse & ~must_reset, normal_only=must_reset & close)


def check_disocclusion(run, mode, W, H, name, tol=TOL_PX):
    cur_kw, prev_kw = DISOCCLUSION
    cur, prev = camera(mode, W, H, **cur_kw), camera(mode, W, H, **prev_kw)
    world_cur, world_prev, min_reset, max_undecided, min_normal_only = disocclusion_worlds()[name]
    cf, pf = frame(cur, world_cur), frame(prev, world_prev)
    pf["depth"] = pf["t"]
    k = classify_disocclusion(prev, cf, pf)
    n_in = int(k["inside"].sum())
    fig = dict(inside=n_in, must_reuse=int(k["must_reuse"].sum()), must_reset=int(k["must_reset"].sum()),
               undecided=int(k["undecided"].sum()), normal_only=int(k["normal_only"].sum()))
    print("disocclusion", name, mode, W, H, fig)
    assert n_in >= W * H / 2
    assert fig["normal_only"] >= min_normal_only, fig
    if (W, H) in CAPPED_SIZES:
        assert fig["must_reset"] >= min_reset, fig
        assert max_undecided is None or fig["undecided"] <= max_undecided * n_in, fig
    res = run(mode, W, H, cur_kw, prev_kw, _bufs(*features(cf), coordinate_history(pf), *features(pf)))
    rec = recovered(res.out)
    _all_full(res, k["must_reuse"])
    err = np.maximum(np.abs(rec[..., 0] - k["bx"]), np.abs(rec[..., 1] - k["by"]))[k["must_reuse"]]
    assert err.max() <= tol, float(err.max())
    _all_reset(res, k["must_reset"])
    has = res.out[..., 3] > 1.0
    assert has[k["must_reuse"]].all() and fig["must_reuse"] >= n_in / 2
    wrong = has & (np.abs(rec[..., 2] - cf["sid"]) > 1e-3)
    assert not wrong.any(), ("history across the silhouette", np.argwhere(wrong)[:5].tolist(), rec[..., 2][wrong][:5])
    fig["straddling"] = int((has & k["undecided"]).sum())
    print("  undecided pixels with a history:", fig["straddling"])
    if name == "hinge-static":           # footprints across the edge: a history, and of their own surface only
        assert fig["straddling"] >= 8, fig
    return fig


# ---- variance, blend, gamma ---------------------------------------------------------------

def check_variance(run, mode, W, H, tol=TOL_VAR):
    """plane world, constant history variance v and frame variance var: out_var = (v sum(w^2) /
    sum(w)^2 N0^2 + var) / (N0 + 1)^2 with the reference's own weights -- all four (sum(w) = 1)
    for a pixel that lands inside, and those of the taps in the image for one that lands in the
    rim up to a pixel outside it, where sum(w) < 1 tells sw^2 from sw."""
    cur_kw, prev_kw = pairs(mode)["all"]
    cur, prev = camera(mode, W, H, **cur_kw), camera(mode, W, H, **prev_kw)
    world = WorldPlane()
    cf, pf = frame(cur, world), frame(prev, world)
    bx, by, _, inside = landing(prev, cf)
    x0, y0 = np.floor(bx), np.floor(by)
    fx, fy = bx - x0, by - y0
    sw, sw2 = np.zeros((H, W)), np.zeros((H, W))
    for dx, dy, w in ((0, 0, (1 - fx) * (1 - fy)), (1, 0, fx * (1 - fy)), (0, 1, (1 - fx) * fy), (1, 1, fx * fy)):
        ok = (x0 + dx >= 0) & (x0 + dx <= W - 1) & (y0 + dy >= 0) & (y0 + dy <= H - 1)
        sw += np.where(ok, w, 0.0)
        sw2 += np.where(ok, w * w, 0.0)
    # the rim: away from the integers, so that the taps offered are not in doubt, and with a quarter
    # of the weight at least, which bounds what a coordinate error of TOL_PX / 8 does to the quotient
    away = lambda f: (f > 1e-3) & (f < 1.0 - 1e-3)   # noqa: E731
    rim = ~inside & (bx > -1.0) & (bx < W) & (by > -1.0) & (by < H) & away(fx) & away(fy) & (sw >= 0.25)
    assert np.abs(sw[inside] - 1.0).max() < 1e-12 and rim.sum() >= 8 and (sw[rim] < 0.999).all(), int(rim.sum())
    v, var = np.array([0.04, 0.01, 0.025]), np.array([0.3, 0.2, 0.1])
    with np.errstate(all="ignore"):
        expect = (v * (sw2 / (sw * sw))[..., None] * N0 * N0 + var) / (N0 + 1.0) ** 2
    z = np.zeros((H, W, 1))
    full = lambda a: np.concatenate([np.broadcast_to(a, (H, W, 3)), z], -1).astype(f32)   # noqa: E731
    res = run(mode, W, H, cur_kw, prev_kw, _bufs(*features(cf), coordinate_history(pf), *features(pf), var=full(var),
                                                 hist_var=full(v)))
    _all_full(res, inside | rim)
    near_half = inside & (np.abs(fx - 0.5) < 0.2) & (np.abs(fy - 0.5) < 0.2)
    assert near_half.sum() >= 20                     # where a wrong power of w moves the value most
    rel = np.abs(res.out_var[..., :3] - expect) / expect
    fig = dict(inside=int(inside.sum()), rim=int(rim.sum()), worst_rel=float(rel[inside].max()),
               worst_rel_rim=float(rel[rim].max()))
    print("variance", mode, W, H, fig)
    assert rel[inside | rim].max() <= tol and (res.out_var[..., 3] == 0).all(), fig
    return fig


def check_blend(run, mode, W=16, H=16, frames=6, max_history=4, tol=TOL_BLEND):
    """equal cameras inside the shell, spatially constant colours and variances: N runs 1, 2, 3,
    4, 4, 4 and the colour follows the float64 recurrence in every pixel -- sc / sw of a constant
    does not depend on the weights.  The variance does: sv / sw^2 of a constant is v sum(w^2) /
    sw^2, and a pixel that lands d of a pixel off its own centre (float32 rounding: d < 2e-6
    measured) has sum(w^2) = 1 - 2 d.  So the variance follows its recurrence to `tol` in the pixels
    that land on themselves exactly (one tap of weight 1; the same pixels in every frame, at least
    a quarter of them), and in the others from below within 4 TOL_PX per frame more."""
    cam_kw = dict(eye=(0.0, 5.0, 17.0), direction=(0.1, -0.05, -1.0), up=(0.05, 1.0, 0.0))
    cam = camera(mode, W, H, **cam_kw)
    fr = frame(cam, WorldShell(cam["eye"]))
    ac, nd = features(fr)
    rng = np.random.default_rng(17)
    cols, vars_ = rng.random((frames, 3)) + 0.1, rng.random((frames, 3)) * 0.05 + 0.01
    z = np.zeros((H, W, 1))
    full = lambda a, w=z: np.concatenate([np.broadcast_to(a, (H, W, 3)), w], -1).astype(f32)   # noqa: E731
    hist, hvar = full(cols[0], z + 1.0), full(vars_[0])
    n, mean, v = 1.0, cols[0].copy(), vars_[0].copy()
    lengths, exact = [n], None
    for k in range(1, frames):
        res = run(mode, W, H, cam_kw, cam_kw, _bufs(ac, nd, hist, ac, nd, color=full(cols[k])[..., :3].copy(),
                                                    var=full(vars_[k]), hist_var=hvar), max_history=max_history)
        ne = min(n, max_history - 1.0)
        mean = (mean * ne + cols[k]) / (ne + 1.0)
        v = (v * ne * ne + vars_[k]) / (ne + 1.0) ** 2
        n = ne + 1.0
        lengths.append(n)
        assert (res.cls == BILINEAR).all() and (res.used == res.offered).all()
        assert exact is None or np.array_equal(exact, res.used == 1)
        exact = res.used == 1
        assert exact.sum() >= W * H / 4, int(exact.sum())
        assert (res.out[..., 3] == n).all(), (k, n, np.unique(res.out[..., 3]))
        assert (np.abs(res.out[..., :3] - mean) <= tol * mean).all(), (k, "colour")
        dv = (res.out_var[..., :3] - v) / v
        assert (np.abs(dv[exact]) <= tol).all(), (k, "variance", float(np.abs(dv[exact]).max()))
        assert (dv <= tol).all() and (dv >= -tol - 4.0 * TOL_PX * k).all(), (k, "variance", float(dv.min()), float(dv.max()))
        assert (res.out_var[..., 3] == 0).all()
        hist, hvar = res.out, res.out_var
    assert lengths == [1, 2, 3, 4, 4, 4]
    return dict(lengths=lengths, exact=int(exact.sum()), variance_low=float(dv.min()))


def check_gamma(run, mode, W=16, H=16, tol=TOL_BLEND):
    """gamma_space: this frame's colour enters as c^2.2, the history as it is"""
    cam_kw = dict(eye=(0.0, 5.0, 17.0))
    cam = camera(mode, W, H, **cam_kw)
    fr = frame(cam, WorldShell(cam["eye"]))
    ac, nd = features(fr)
    rng = np.random.default_rng(29)
    color = (rng.random((H, W, 3)) * 0.98 + 0.01).astype(f32)
    h = rng.random(3) + 0.1
    hist = np.concatenate([np.broadcast_to(h, (H, W, 3)), np.full((H, W, 1), 3.0)], -1).astype(f32)
    res = run(mode, W, H, cam_kw, cam_kw, _bufs(ac, nd, hist, ac, nd, color=color), gamma_space=True)
    expect = (h.astype(f32).astype(f64) * 3.0 + color.astype(f64) ** 2.2) / 4.0
    assert (res.out[..., 3] == 4.0).all()
    rel = np.abs(res.out[..., :3] - expect) / expect
    assert rel.max() <= tol, float(rel.max())
    return dict(worst_rel=float(rel.max()))


# ---- the renderer's own frames ---------------------------------------------------------------

def centre_rays(mode, W, H, cam_kw):
    """the reference's pixel-centre rays as the closest-hit queries take them: (H, W, 3) float32 each"""
    ys, xs = np.mgrid[0:H, 0:W]
    o, d = pixel_ray(camera(mode, W, H, **cam_kw), xs, ys)
    return o.astype(f32), d.astype(f32)


def fit_centre(albedo_cov, normal_depth, t_c, hit_c):
    """Least squares of z - t_c = a + ox dt_c/dx + oy dt_c/dy over the pixels all of whose samples
    hit one smooth surface (coverage 1, |mean normal|^2 > 0.9999), whose 3 x 3 neighbours do too,
    border excluded: z the renders' mean depth, t_c the depth along the reference's centre ray.
    A pixel centre off by (ox, oy) pixels shows as that slope, a depth measured from another
    origin as the offset a.  Returns (ox, oy, a, pixels, standard errors)."""
    ac, nd = np.asarray(albedo_cov, f64), np.asarray(normal_depth, f64)
    H, W = t_c.shape
    good = (ac[..., 3] == 1.0) & ((nd[..., :3] ** 2).sum(-1) > 0.9999) & hit_c
    block = np.zeros((H, W), bool)
    block[1:-1, 1:-1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            block[1:-1, 1:-1] &= good[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]
    t = np.asarray(t_c, f64)
    gx, gy = np.zeros((H, W)), np.zeros((H, W))
    gx[:, 1:-1] = (t[:, 2:] - t[:, :-2]) / 2.0
    gy[1:-1, :] = (t[2:, :] - t[:-2, :]) / 2.0
    A = np.stack([np.ones(int(block.sum())), gx[block], gy[block]], -1)
    y = (nd[..., 3] - t)[block]
    sol, *_ = np.linalg.lstsq(A, y, rcond=None)
    resid = y - A @ sol
    cov = np.linalg.inv(A.T @ A) * (resid @ resid) / max(len(y) - 3, 1)
    a, ox, oy = sol
    return float(ox), float(oy), float(a), int(block.sum()), np.sqrt(np.diag(cov))[[1, 2, 0]]


def check_centre_fit(albedo_cov, normal_depth, t_c, hit_c, what=""):
    ox, oy, a, n, se = fit_centre(albedo_cov, normal_depth, t_c, hit_c)
    print(f"centre fit {what}: ox {ox:+.4f} oy {oy:+.4f} a {a:+.4f} over {n} pixels, standard errors {se.round(4).tolist()}")
    assert n >= 150, n
    assert abs(ox) < 0.25 and abs(oy) < 0.25 and abs(a) < 0.25, (ox, oy, a)
    return dict(ox=ox, oy=oy, a=a, pixels=n)

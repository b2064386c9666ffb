"""Ray families for the closest-hit pins.

ray_sets: seven adversarial families inside the scene's root box, unit
directions (tests/test_brute_pins.py on the CPU oracle, tests/test_gpu_*.py on
the device).  With k = n // 8, in this order: 1 random rays (2k), 2 rays aimed
at triangle interiors (2k), 3 axis-parallel rays (k), 4 origins exactly on KD
split planes (k), 5 origins on triangle edges (k, indices [6k, 7k)), 6 rays
grazing a triangle's plane (k), 7 rays through vertices (k + n % 8): 9k + n % 8
rays.  `families=True` also returns the family number of every ray.

contract_ray_sets: what the ray entries' contract (include/mcpt.h: finite
origins; every direction component zero, of either sign, or with a finite
reciprocal) allows beyond that -- signed zeros, origins outside the root box and
exactly on box faces, directions of any length -- and subnormal components,
which lie outside it.
"""
import numpy as np

EDGE_ORIGINS = 5          # ray_sets family whose brute-force differences are float artifacts
VERTEX_RAYS = 7


def _box(s):
    nodes = s.kd_nodes()
    return nodes, nodes[0, 4:7].view(np.float32), nodes[0, 7:10].view(np.float32)


def _unit(v):
    v = v.astype(np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def ray_sets(s, n, seed, families=False):
    """9 * (n // 8) + n % 8 rays (origins, directions float32) over the scene's root box in seven
    families (module docstring); families=True: (origins, directions, family 1..7 per ray).
    The first 8 * (n // 8) rays depend on (scene, n, seed) alone; the vertex family is drawn last."""
    r = np.random.default_rng(seed)
    nodes, bmin, bmax = _box(s)
    ext = bmax - bmin
    kv = s.kd_verts()                                     # (nkd, 3, 3) float32
    k = n // 8
    unit = _unit

    def in_box(m):
        return (bmin + ext * r.random((m, 3))).astype(np.float32)

    def tri_points(m, tris=None):
        t = r.integers(0, kv.shape[0], m) if tris is None else tris
        a, b = r.random(m), r.random(m)
        sw = a + b > 1
        a[sw], b[sw] = 1 - a[sw], 1 - b[sw]
        v = kv[t].astype(np.float64)
        return (v[:, 0] + a[:, None] * (v[:, 1] - v[:, 0]) + b[:, None] * (v[:, 2] - v[:, 0])).astype(np.float32), t

    O, D = [], []
    # 1 random rays
    O.append(in_box(2 * k)); D.append(unit(r.standard_normal((2 * k, 3))))
    # 2 aimed at triangle interiors
    o = in_box(2 * k); p, _ = tri_points(2 * k)
    O.append(o); D.append(unit(p - o))
    # 3 axis-parallel: one or two zero components (the dir == 0 slab paths)
    d = r.standard_normal((k, 3))
    z = r.integers(0, 3, k)
    d[np.arange(k), z] = 0.0
    two = r.random(k) < 0.5
    d[np.arange(k)[two], (z[two] + 1) % 3] = 0.0
    O.append(in_box(k)); D.append(unit(d))
    # 4 origins exactly on KD split planes, inside the node's box
    inner = np.nonzero(nodes[:, 2])[0]
    pick = inner[r.integers(0, inner.size, k)]
    nb0, nb1 = nodes[pick, 4:7].view(np.float32), nodes[pick, 7:10].view(np.float32)
    o = (nb0 + (nb1 - nb0) * r.random((k, 3))).astype(np.float32)
    ax = nodes[pick, 2].astype(np.int64) - 1
    o[np.arange(k), ax] = nodes[pick, 3].view(np.float32)
    half = k // 2
    p, _ = tri_points(k)
    d = unit(r.standard_normal((k, 3)))
    d[:half] = unit(p[:half] - o[:half])
    O.append(o); D.append(d)
    # 5 origins on triangle edges; half toward the opposite vertex (in the triangle's plane)
    t = r.integers(0, kv.shape[0], k)
    e = r.integers(0, 3, k)
    a = kv[t, e].astype(np.float64); b = kv[t, (e + 1) % 3].astype(np.float64); c = kv[t, (e + 2) % 3]
    o = (a + r.random((k, 1)) * (b - a)).astype(np.float32)
    d = unit(r.standard_normal((k, 3)))
    d[:half] = unit(c[:half].astype(np.float64) - o[:half])
    O.append(o); D.append(d)
    # 6 grazing: in the plane of a triangle (direction along one of its edges), origin
    #   a tiny distance off the plane or on it, aimed across the triangle
    t = r.integers(0, kv.shape[0], k)
    v = kv[t].astype(np.float64)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    cen = v.mean(axis=1)
    edge = v[:, 1] - v[:, 0]
    off = r.choice([0.0, 1e-6, -1e-6, 1e-4], size=(k, 1))
    o = (cen - 2.0 * edge + off * nrm).astype(np.float32)
    O.append(o); D.append(unit(edge))
    # 7 through vertices (drawn last: the rays above do not depend on this family's size)
    rest = k + n % 8
    o = in_box(rest)
    vv = kv[r.integers(0, kv.shape[0], rest), r.integers(0, 3, rest)]
    O.append(o); D.append(unit(vv.astype(np.float64) - o))
    fam = np.concatenate([np.full(x.shape[0], i, np.int32) for i, x in enumerate(O, 1)])
    O, D = np.concatenate(O), np.concatenate(D)
    ok = np.isfinite(D).all(axis=1) & (np.abs(D).sum(axis=1) > 0)
    if families:
        return O[ok], D[ok], fam[ok]
    return O[ok], D[ok]


# ---- the rest of the contract ---------------------------------------------------

FAM_A, FAM_B, FAM_C, FAM_D, FAM_E = range(5)
FAMILY_NAMES = ("A signed zeros", "B outside origins", "C origins on faces", "D powers of two", "E subnormal")
SCALE_EXPONENTS = (-40, -20, 20, 40)
# sub-families (info["sub"])
A_INSIDE, A_OUT_ZERO_AXIS, A_OUT_OTHER_AXIS = 0, 1, 2
B_AIMED, B_PASS_BY, B_CORNER, B_AWAY = 0, 1, 2, 3
C_ROOT, C_NODE, C_NODE_F16 = 0, 1, 2
E_ONE, E_ALL = 0, 1


def root_box_miss(s, o, d):
    """The ordered walk's root-interval test (oracle/render_ref.c isect_kd_ordered's prologue,
    csrc/trace_device.hpp begin_ray) in float32: True where the ray leaves before any node visit."""
    f = np.float32
    _, bmin, bmax = _box(s)
    eps_hi = f(1.000244140625)
    with np.errstate(all="ignore"):
        inv = f(1) / d
        z = d == 0
        miss = (z & ((o < bmin) | (o > bmax))).any(axis=1)
        t0, t1 = (bmin - o) * inv, (bmax - o) * inv
        lo, hi = np.where(d < 0, t1, t0), np.where(d < 0, t0, t1)
        tmin = np.zeros(o.shape[0], f)
        tmax = np.full(o.shape[0], np.finfo(f).max, f)
        for a in range(3):
            nz = ~z[:, a]
            tmin = np.where(nz & (lo[:, a] > tmin), lo[:, a], tmin)
            tmax = np.where(nz & (hi[:, a] < tmax), hi[:, a], tmax)
        return miss | (tmin > tmax * eps_hi)


def contract_ray_sets(s, n, seed, info=False):
    """5 * (n // 5) rays in five families of n // 5 (FAM_A..FAM_E per ray in the third result),
    each from fresh draws; no origin lies on a triangle edge except in D's copies of such rays.

    A  signed zeros: axis-parallel rays, one or two zero components, each +0.0 or -0.0 at
       random; half the origins inside the root box, a quarter outside it along a zero axis
       (the walk's slab-containment miss), a quarter outside along a non-zero axis.
    B  outside origins, half up to 3 extents and half 3 to 100 extents from the box: aimed at
       points inside it (40%), aimed to pass it by (22%), aimed at its corners, exactly or a
       little off (16%), pointing away (22%).
    C  origins exactly on a face of the root box, of a KD node's box (kd_nodes()[:, 4:10]) or
       of that box rounded outward to binary16 (the child-box cull's bounds), a third each;
       the direction's component along the face's axis is +-0.0, inward or outward, a third each.
    D  n // 20 rays spread over ray_sets(s, ., seed + 1), through-vertex rays included, with
       the directions times 2^k, k = -40, -20, 20, 40 (exact), scale by scale in that order.
    E  subnormal components, outside the contract (the walk's answer is defined, the brute
       force's is not reproduced: tests/test_ray_contract_cpu.py): half with one subnormal
       component beside normal ones, half with all three subnormal.
    A-C have unit directions; E's first half has up to rounding.

    Checked by tests/test_ray_contract_cpu.py with the oracle at n = 15 000 and 40 000 on
    scene01 (both trees) and scene03, and at 40 000 on the 70k-triangle mesh: every family
    holds at least 2000 rays; at least 500 rays of A and 1000 of B leave at the root box (no
    node visit); at least 30% of B hit and at least 5% miss; at least 500 origins of C equal
    their bound exactly in float32.

    info=True adds a dict: sub (sub-family per ray, the constants above), scale_exp (k for D,
    else 0), exempt (D's copies of ray_sets family 5: origins on triangle edges), base_o /
    base_d (D's unscaled rays, n // 20), axis / bound (C's face: axis and float32 bound, else
    -1 / 0)."""
    import oracle
    r = np.random.default_rng(seed)
    nodes, bmin, bmax = _box(s)
    ext = (bmax - bmin).astype(np.float64)
    cen = (bmin.astype(np.float64) + bmax) / 2
    kv = s.kd_verts()
    m = n // 5
    f32 = np.float32

    def in_box(c):
        return (bmin + ext * r.random((c, 3))).astype(f32)

    def signed_zero(c):
        return np.where(r.random(c) < 0.5, 0.0, -0.0)

    def split(c, fractions):
        """sub-family numbers 0.. with the given fractions of c rays, in blocks"""
        edges = np.rint(np.cumsum(fractions) * c).astype(int)
        return np.searchsorted(edges, np.arange(c), side="right").clip(max=len(fractions) - 1)

    O, D, SUB = [], [], []
    rows = np.arange(m)

    # A signed zeros
    d = r.standard_normal((m, 3))
    z = r.integers(0, 3, m)
    two = r.random(m) < 0.5
    z2 = (z + 1 + r.integers(0, 2, m)) % 3                # a second axis, zero for `two`
    d[rows, z] = signed_zero(m)
    d[rows[two], z2[two]] = signed_zero(int(two.sum()))
    nzero = np.where(two, 3 - z - z2, (z + 1 + r.integers(0, 2, m)) % 3)   # an axis with d != 0
    sub = split(m, [0.5, 0.25, 0.25])
    o = in_box(m).astype(np.float64)
    dist = ext * (0.01 + 2.99 * r.random((m, 1)))
    side = r.random(m) < 0.5
    for which, axis in ((A_OUT_ZERO_AXIS, z), (A_OUT_OTHER_AXIS, nzero)):
        sel = rows[sub == which]
        a = axis[sel]
        o[sel, a] = np.where(side[sel], bmin[a] - dist[sel, a], bmax[a] + dist[sel, a])
    O.append(o.astype(f32)); D.append(_unit(d)); SUB.append(sub)

    # B outside origins
    sub = split(m, [0.40, 0.22, 0.16, 0.22])
    far = r.random(m) < 0.5
    dist = np.where(far, np.exp(r.uniform(np.log(3.0), np.log(100.0), m)), r.uniform(0.05, 3.0, m))
    out_axes = r.random((m, 3)) < 0.5
    out_axes[rows, r.integers(0, 3, m)] = True            # outside along one to three axes
    low = r.random((m, 3)) < 0.5
    o = in_box(m).astype(np.float64)
    o = np.where(out_axes, np.where(low, bmin - dist[:, None] * ext, bmax + dist[:, None] * ext), o).astype(f32)
    o64 = o.astype(np.float64)
    tri = r.integers(0, kv.shape[0], m)
    w = r.dirichlet((1.0, 1.0, 1.0), m)
    on_tri = (kv[tri].astype(np.float64) * w[:, :, None]).sum(axis=1)
    target = np.where((r.random(m) < 0.6)[:, None], on_tri, in_box(m).astype(np.float64))
    # pass by: a point on a sphere around the box, 1.05 to 3 circumscribed radii out
    radius = np.linalg.norm(ext) / 2
    shell = cen + _unit(r.standard_normal((m, 3))).astype(np.float64) * radius * r.uniform(1.05, 3.0, (m, 1))
    corner = np.where(r.random((m, 3)) < 0.5, bmin, bmax).astype(np.float64)
    corner += np.where((r.random(m) < 0.25)[:, None], 0.0, ext * r.uniform(-0.05, 0.05, (m, 3)))
    away = o64 + (o64 - cen) + ext * r.standard_normal((m, 3)) * 0.2
    target = np.select([(sub == B_AIMED)[:, None], (sub == B_PASS_BY)[:, None], (sub == B_CORNER)[:, None]],
                       [target, shell, corner], away)
    O.append(o); D.append(_unit(target - o64)); SUB.append(sub)

    # C origins on faces
    sub = split(m, [1 / 3, 1 / 3, 1 / 3])
    lo_all, hi_all = nodes[:, 4:7].view(f32), nodes[:, 7:10].view(f32)
    proper = np.nonzero((lo_all < hi_all).all(axis=1))[0]  # (an empty node's box is inverted)
    pick = np.where(sub == C_ROOT, 0, proper[r.integers(0, proper.size, m)])
    nb0, nb1 = lo_all[pick], hi_all[pick]
    o = (nb0 + (nb1.astype(np.float64) - nb0) * r.random((m, 3))).astype(f32)
    axis = r.integers(0, 3, m)
    upper = r.random(m) < 0.5
    bound = np.where(upper, nb1[rows, axis], nb0[rows, axis]).astype(f32)
    h = sub == C_NODE_F16
    bound[h & upper] = oracle.f16_outward(bound[h & upper], +1)
    bound[h & ~upper] = oracle.f16_outward(bound[h & ~upper], -1)
    o[rows, axis] = bound
    d = r.standard_normal((m, 3))
    kind = r.integers(0, 3, m)                            # 0: in the face's plane, 1: inward, 2: outward
    mag = np.abs(d[rows, axis])
    inward = np.where(upper, -mag, mag)
    d[rows, axis] = np.select([kind == 0, kind == 1], [signed_zero(m), inward], -inward)
    O.append(o); D.append(_unit(d)); SUB.append(sub)

    # D powers of two
    q = m // 4
    bo, bd, bf = ray_sets(s, 8 * q, seed + 1, families=True)
    sel = np.arange(q) * (bo.shape[0] // q)
    bo, bd, bf = np.ascontiguousarray(bo[sel]), np.ascontiguousarray(bd[sel]), bf[sel]
    scale_exp = np.zeros(5 * m, np.int32)
    exempt = np.zeros(5 * m, bool)
    for i, e in enumerate(SCALE_EXPONENTS):
        dk = np.ldexp(bd, e).astype(f32)
        assert np.array_equal(np.ldexp(dk, -e), bd), "a scaled component left the normal range"
        O.append(bo); D.append(dk); SUB.append(np.full(q, i))
        scale_exp[3 * m + i * q:3 * m + (i + 1) * q] = e
        exempt[3 * m + i * q:3 * m + (i + 1) * q] = bf == EDGE_ORIGINS
    pad = m - 4 * q                                       # (m not a multiple of 4: plain copies)
    if pad:
        O.append(bo[:pad]); D.append(bd[:pad]); SUB.append(np.full(pad, len(SCALE_EXPONENTS)))
        exempt[3 * m + 4 * q:4 * m] = bf[:pad] == EDGE_ORIGINS

    # E subnormal components
    def subnormal(c):
        mant = np.floor(2.0 ** r.uniform(0.0, 23.0, c)).astype(np.uint32).clip(1, 2**23 - 1)
        return (mant | (r.integers(0, 2, c).astype(np.uint32) << 31)).view(f32)
    sub = split(m, [0.5, 0.5])
    d = _unit(r.standard_normal((m, 3)))
    d[rows, r.integers(0, 3, m)] = subnormal(m)
    d[sub == E_ALL] = subnormal(3 * int((sub == E_ALL).sum())).reshape(-1, 3)
    o = in_box(m)
    outside = rows[r.random(m) < 0.25]
    a = r.integers(0, 3, outside.size)
    o[outside, a] = (bmin[a] - ext[a] * r.uniform(0.01, 3.0, outside.size)).astype(f32)
    O.append(o); D.append(d); SUB.append(sub)

    o, d = np.concatenate(O), np.concatenate(D)
    fam = np.repeat(np.arange(5, dtype=np.int32), m)
    assert o.shape == d.shape == (5 * m, 3) and np.isfinite(o).all() and np.isfinite(d).all()
    assert (d != 0).any(axis=1).all()
    if not info:
        return o, d, fam
    c_axis = np.full(5 * m, -1, np.int32)
    c_bound = np.zeros(5 * m, f32)
    c_axis[2 * m:3 * m], c_bound[2 * m:3 * m] = axis, bound
    return o, d, fam, dict(sub=np.concatenate(SUB).astype(np.int32), scale_exp=scale_exp, exempt=exempt,
                           base_o=bo, base_d=bd, axis=c_axis, bound=c_bound)

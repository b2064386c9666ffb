"""The ray entries' contract on the CPU oracle (include/mcpt.h, "Ray
preconditions"): finite origins anywhere, directions of any length whose
components are zero -- of either sign -- or have a finite float reciprocal.

tests/_raysets.py contract_ray_sets sends what the seven families of ray_sets
never do: -0.0 components (A), origins outside the root box (B), origins
exactly on the faces of the root box, of KD node boxes and of their binary16
forms (C), directions times 2^-40 .. 2^40 (D) and, outside the contract,
subnormal components (E).  Here the ordered walk, with the child-box cull on
and off, is held to the brute force on A-D bit for bit, to its own answers
under scaling (a pin that does not depend on the oracle's arithmetic: any
absolute epsilon in the walk would break it), and on E to termination and
determinism alone.  tests/test_gpu_ray_contract.py holds the kernels to the
same walk.

Why E is outside the contract: scene01, origin (5.462696, 9.76097,
0.66874343), direction (0, 8.24867e-40, 0).  The brute force hits triangle 0 at
t = 2.9e38 < FLT_MAX; the walk misses, because 1 / d = +inf makes every
split-plane t infinite and no far child is ever entered.  A component must be
zero or have a finite reciprocal (|d| >= 2^-126 suffices);
test_a_subnormal_component_is_outside_the_contract keeps the example.
"""
import os

import numpy as np
import pytest

import _raysets as R
from _exact_hits import float_artifact

THREADS = min(os.cpu_count() or 8, 16)
N_GPU, N = 15_000, 40_000                 # tests/test_gpu_ray_contract.py's n, and the n of the pins here
SEED = 41
VISITS = ("inner_visits", "leaf_visits", "leaf_refs", "tri_tests")
CONFIGS = [("scene01", "reference"), ("scene03", "reference"), ("cornell_bunny70k", "reference"), ("scene01", "sah")]
IDS = [f"{n}-{kd}" if kd != "reference" else n for n, kd in CONFIGS]


class Ctx:
    def __init__(self, oracle_mod):
        self.orc = oracle_mod
        self._scene, self._rays = {}, {}

    def scene(self, cfg):
        if cfg not in self._scene:
            from montecarlopathtracer_amd.scenes import scene_path
            self._scene[cfg] = self.orc.Scene(scene_path(cfg[0]), kd_build=cfg[1])
        return self._scene[cfg]

    def rays(self, cfg, n=N):
        if (cfg, n) not in self._rays:
            self._rays[(cfg, n)] = R.contract_ray_sets(self.scene(cfg), n, SEED, info=True)
        return self._rays[(cfg, n)]

    def walk(self, cfg, o, d, boxes):
        return self.scene(cfg).intersect(o, d, self.orc.KD_ORDERED, node_boxes=boxes, threads=THREADS)


@pytest.fixture(scope="module")
def ctx(oracle_mod):
    return Ctx(oracle_mod)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the generators ---------------------------------------------------------------

def test_every_family_of_ray_sets_holds_k_rays(ctx):
    """ray_sets gave its last family n - 8 * (n // 8) rays: none at every n the suite uses."""
    s = ctx.scene(CONFIGS[0])
    for n in (100_000, 60_000, 40_000, 20_000, 100_007):
        k = n // 8
        o, d, fam = R.ray_sets(s, n, 17, families=True)
        assert o.shape[0] == d.shape[0] == fam.shape[0] == 9 * k + n % 8      # (scene01: no ray dropped)
        counts = np.bincount(fam, minlength=8)
        assert counts[0] == 0 and (counts[1:] >= k).all(), (n, counts)
        assert counts[R.VERTEX_RAYS] == k + n % 8
        assert (np.diff(fam) >= 0).all()                                      # families in order
        assert (fam[6 * k:7 * k] == R.EDGE_ORIGINS).all() and (fam == R.EDGE_ORIGINS).sum() == k
        o2, d2 = R.ray_sets(s, n, 17)
        assert np.array_equal(_bits(o), _bits(o2)) and np.array_equal(_bits(d), _bits(d2))
    # the vertex family is drawn last: its size does not move the rays before it
    a, b = R.ray_sets(s, 100_000, 17), R.ray_sets(s, 100_007, 17)
    k8 = 8 * (100_000 // 8)
    assert np.array_equal(_bits(a[0][:k8]), _bits(b[0][:k8])) and np.array_equal(_bits(a[1][:k8]), _bits(b[1][:k8]))
    # through-vertex rays do go through vertices: the exact ray meets a vertex of the scene
    kv = s.kd_verts().reshape(-1, 3).astype(np.float64)
    v = fam == R.VERTEX_RAYS
    oo, dd = o[v][:200].astype(np.float64), d[v][:200].astype(np.float64)
    rel = kv[None, :, :] - oo[:, None, :]
    off = np.linalg.norm(np.cross(rel, dd[:, None, :]), axis=2).min(axis=1)
    assert (off < 1e-4).all(), off.max()


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
@pytest.mark.parametrize("n", [N_GPU, N])
def test_contract_families_meet_their_stated_conditions(ctx, cfg, n):
    s = ctx.scene(cfg)
    o, d, fam, info = ctx.rays(cfg, n)
    assert o.dtype == d.dtype == np.float32 and np.isfinite(o).all() and np.isfinite(d).all()
    assert (np.bincount(fam, minlength=5) >= 2000).all()
    # root-box misses: the float32 restatement of the prologue, checked against the oracle's counters
    miss = R.root_box_miss(s, o, d)
    tk, _, _, ck = ctx.walk(cfg, o[miss], d[miss], 0)
    assert ck["inner_visits"] == ck["leaf_visits"] == 0 and (tk == -1).all()
    _, _, _, ck = ctx.walk(cfg, o[~miss], d[~miss], 0)
    assert ck["inner_visits"] >= int((~miss).sum())       # every other ray visits the root at least
    tk, _, _, _ = ctx.walk(cfg, o, d, 0)
    hit = tk >= 0
    a, b, c, dfam, e = (fam == f for f in range(5))
    sub = info["sub"]
    print(cfg, n, "rays", np.bincount(fam).tolist(), "hit fractions", [round(float(hit[fam == f].mean()), 3) for f in range(5)],
          "root-box misses", [int(miss[fam == f].sum()) for f in range(5)])
    # A: signed zeros of both signs, every outside-along-a-zero-axis ray a root miss
    za = a[:, None] & (d == 0)
    assert (za & np.signbit(d)).sum() >= 500 and (za & ~np.signbit(d)).sum() >= 500
    assert za.sum(axis=1)[a].min() >= 1 and za.sum(axis=1)[a].max() == 2
    assert miss[a & (sub == R.A_OUT_ZERO_AXIS)].all()
    assert (miss & a).sum() >= 500
    assert 0.3 < hit[a & (sub == R.A_INSIDE)].mean()
    # B: all origins outside the root box
    nodes = s.kd_nodes()
    bmin, bmax = nodes[0, 4:7].view(np.float32), nodes[0, 7:10].view(np.float32)
    assert ((o[b] < bmin) | (o[b] > bmax)).any(axis=1).all()
    assert (miss & b).sum() >= 1000
    assert hit[b].mean() >= 0.30 and (~hit[b]).mean() >= 0.05
    for sb in (R.B_AIMED, R.B_PASS_BY, R.B_CORNER):
        assert hit[b & (sub == sb)].any() and (sub[b] == sb).sum() >= 300
    far = np.maximum(np.maximum(bmin - o, o - bmax), 0).max(axis=1) > 50 * (bmax - bmin).min()
    assert (far & b & hit).sum() >= 100                   # hits from 50 extents and more away
    # C: the origin's coordinate is the bound, exactly
    rows = np.nonzero(c)[0]
    assert (o[rows, info["axis"][rows]] == info["bound"][rows]).sum() >= 500
    assert (o[rows, info["axis"][rows]] == info["bound"][rows]).all()
    dz = d[rows, info["axis"][rows]]
    assert (dz == 0).sum() >= 500 and (dz > 0).sum() >= 500 and (dz < 0).sum() >= 500
    assert (np.signbit(dz) & (dz == 0)).any() and (~np.signbit(dz) & (dz == 0)).any()
    for sb in (R.C_ROOT, R.C_NODE, R.C_NODE_F16):
        assert (sub[c] == sb).sum() >= 600 and hit[c & (sub == sb)].any()
    assert 0.2 < hit[c].mean() < 0.95
    # D: exact powers of two of unit directions, the exempt rays a minority
    for k in R.SCALE_EXPONENTS:
        m = dfam & (info["scale_exp"] == k)
        assert m.sum() == info["base_o"].shape[0] >= 500
        assert np.array_equal(_bits(d[m]), _bits(np.ldexp(info["base_d"], k)))
        assert np.array_equal(_bits(o[m]), _bits(info["base_o"]))
    assert 0 < info["exempt"].sum() < 0.2 * dfam.sum() and not info["exempt"][~dfam].any()
    # E: subnormal, non-zero components
    tiny = np.finfo(np.float32).tiny
    sn = (np.abs(d) < tiny) & (d != 0)
    assert (sn[e].sum(axis=1) >= 1).all() and not sn[~e].any()
    assert (sn[e & (sub == R.E_ALL)].sum(axis=1) == 3).all() and (sub[e] == R.E_ALL).sum() >= 1000
    # A-D keep the contract: every component zero or with a finite reciprocal
    with np.errstate(all="ignore"):
        assert (np.isfinite(np.float32(1) / d[~e]) | (d[~e] == 0)).all()


# ---- A-D: the ordered walk is the brute force ---------------------------------------

@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_walk_equals_brute_force_on_the_contract_families(ctx, cfg):
    """Bit for bit (triangle, geometry, beta, gamma, t, hit point) on every ray of A-D, cull
    on and off; only D's copies of rays that start on a triangle edge may differ, each
    difference a float artifact by the exact test (no t < 1e-5 shortcut: t is scaled there)."""
    s = ctx.scene(cfg)
    o, d, fam, info = ctx.rays(cfg)
    keep = fam != R.FAM_E
    o, d, exempt = o[keep], d[keep], info["exempt"][keep]
    tb, gb, hb, _ = s.intersect(o, d, ctx.orc.BRUTE, threads=THREADS)
    kv = s.kd_verts()
    for boxes in (0, 1):
        tk, gk, hk, _ = ctx.walk(cfg, o, d, boxes)
        bad = np.nonzero((tb != tk) | (gb != gk) | (_bits(hb) != _bits(hk)).any(axis=1))[0]
        assert exempt[bad].all(), (cfg, boxes, bad[~exempt[bad]][:10], fam[keep][bad[~exempt[bad]]][:10])
        assert bad.size <= 50, (cfg, boxes, bad.size)
        for i in bad:
            assert float_artifact(kv, o[i], d[i], tb[i], hb[i], tk[i], hk[i], origin_shortcut=False), \
                (cfg, boxes, i, tb[i], tk[i])


# ---- D: scale invariance --------------------------------------------------------------

@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_scaling_the_direction_by_a_power_of_two_scales_t_and_nothing_else(ctx, cfg):
    """d * 2^k, k = -40 .. 40: the same triangle, geometry, beta and gamma bits, hit point and
    traversal counters, and t_k == t_0 * 2^-k exactly -- every product and quotient of the
    walk scales exactly, so any absolute constant in it would show."""
    o, d, fam, info = ctx.rays(cfg)
    bo, bd = info["base_o"], info["base_d"]
    for boxes in (0, 1):
        t0, g0, h0, c0 = ctx.walk(cfg, bo, bd, boxes)
        assert 0.3 < (t0 >= 0).mean()
        for k in R.SCALE_EXPONENTS:
            m = (fam == R.FAM_D) & (info["scale_exp"] == k)
            tk, gk, hk, ck = ctx.walk(cfg, o[m], d[m], boxes)
            what = (cfg, boxes, k)
            assert np.array_equal(tk, t0) and np.array_equal(gk, g0), what
            assert np.array_equal(_bits(hk[:, :2]), _bits(h0[:, :2])), what
            assert np.array_equal(_bits(hk[:, 2]), _bits(np.ldexp(h0[:, 2], -k))), what
            assert np.array_equal(_bits(hk[:, 3:]), _bits(h0[:, 3:])), what
            for c in VISITS:
                assert ck[c] == c0[c], (what, c, ck[c], c0[c])


# ---- E: outside the contract ------------------------------------------------------------

@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_subnormal_components_terminate_and_are_deterministic(ctx, cfg):
    """No comparison with the brute force (module docstring): the walk ends, and gives the
    same hits and counters run again, on one thread and on many."""
    o, d, fam, _ = ctx.rays(cfg)
    e = fam == R.FAM_E
    o, d = np.ascontiguousarray(o[e]), np.ascontiguousarray(d[e])
    for boxes in (0, 1):
        a = ctx.walk(cfg, o, d, boxes)
        b = ctx.walk(cfg, o, d, boxes)
        c = ctx.scene(cfg).intersect(o, d, ctx.orc.KD_ORDERED, node_boxes=boxes, threads=1)
        for other in (b, c):
            assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1])
            assert np.array_equal(_bits(a[2]), _bits(other[2]))
            for k in VISITS:
                assert a[3][k] == other[3][k]
        assert np.isfinite(a[2]).all()
        assert (a[0] >= 0).any() and (a[0] < 0).any()


def test_a_subnormal_component_is_outside_the_contract(ctx):
    """The recorded counter-example: the brute force's hit at t = 2.9e38 that the walk, whose
    reciprocal is infinite, does not find -- and does find once the component has a finite
    reciprocal."""
    cfg = CONFIGS[0]
    s = ctx.scene(cfg)
    o = np.array([[5.462696, 9.76097, 0.66874343]], np.float32)
    d = np.array([[0.0, 8.24867e-40, 0.0]], np.float32)
    with np.errstate(all="ignore"):
        assert np.isinf(np.float32(1) / d[0, 1])
    tb, _, hb, _ = s.intersect(o, d, ctx.orc.BRUTE)
    assert tb[0] == 0 and 2.8e38 < hb[0, 2] < np.finfo(np.float32).max
    for boxes in (0, 1):
        tk, _, _, _ = ctx.walk(cfg, o, d, boxes)
        assert tk[0] == -1
    d[0, 1] = 2.0 ** -126
    tb, gb, hb, _ = s.intersect(o, d, ctx.orc.BRUTE)
    for boxes in (0, 1):
        tk, gk, hk, _ = ctx.walk(cfg, o, d, boxes)
        assert tk[0] == tb[0] == 0 and gk[0] == gb[0] and np.array_equal(_bits(hk), _bits(hb))

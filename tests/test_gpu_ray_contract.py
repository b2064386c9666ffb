"""The ray entries on the rays their contract allows and tests/_raysets.py
ray_sets never sends (contract_ray_sets: A signed zeros, B origins outside the
root box, C origins exactly on box faces, D directions times 2^-40 .. 2^40) and
on E, subnormal components, which lie outside it (include/mcpt.h "Ray
preconditions"; tests/test_ray_contract_cpu.py holds the oracle's walk to the
brute force on A-D and records why E is excluded).

mcpt_trace_device, mcpt_intersect (the older query kernel of render.hip),
mcpt_occluded_device, mcpt_occluded and mcpt_radiance_device against the CPU
oracle's ordered walk with the layout's cull -- triangle ids, the bits of
(beta, gamma, t), the four traversal counters -- on every family, E as given;
against the brute force on A-D (D's copies of rays that start on a triangle
edge excepted, as in tests/test_gpu_intersect.py); per-ray and scalar t_max;
batches in which whole waves leave at the root box; one workgroup refilling
over the batch.  15 000 rays per scene, 3000 per family, seed 41.
"""
import numpy as np
import pytest

import _raysets as R
from test_gpu_radiance import query as radiance, same
from test_gpu_rayquery import CONFIGS, COUNTERS, FLT_MAX, _bits, assert_counters, assert_same_hits, occluded, trace

pytestmark = pytest.mark.gpu

N, SEED = 15_000, 41
KEYS = ["scene01", "scene01-global", "scene03", "scene01-sah"]
VISITS = COUNTERS[1:]
f32 = np.float32


class Ctx:
    """scenes, oracle scenes, the ray set of each and the oracle's answers, each made once"""

    def __init__(self, mcpt, oracle_mod):
        self.mcpt, self.oracle = mcpt, oracle_mod
        self._scene, self._oscene, self._rays, self._walk, self._brute = {}, {}, {}, {}, {}

    def scene(self, key):
        if key not in self._scene:
            name, layout, kd = CONFIGS[key]
            self._scene[key] = self.mcpt.Scene(self.mcpt.ObjModel(self.mcpt.scene_path(name)), layout=layout,
                                               kd_build=kd)
        return self._scene[key]

    def boxes(self, key):
        b = int(self.scene(key).info()["node_boxes"])
        assert b == (0 if key in ("scene01", "scene01-sah") else 1)
        return b

    def oscene(self, key):
        name, _, kd = CONFIGS[key]
        if (name, kd) not in self._oscene:
            self._oscene[(name, kd)] = self.oracle.Scene(self.mcpt.scene_path(name), kd_build=kd)
        return self._oscene[(name, kd)]

    def rays(self, key):
        name, _, kd = CONFIGS[key]
        if (name, kd) not in self._rays:
            self._rays[(name, kd)] = R.contract_ray_sets(self.oscene(key), N, SEED, info=True)
        return self._rays[(name, kd)]

    def pick(self, key, mask):
        o, d, _, _ = self.rays(key)
        return np.ascontiguousarray(o[mask]), np.ascontiguousarray(d[mask])

    def walk(self, key, o, d):
        """the oracle's ordered walk with the layout's cull -> (tri, geom, (n, 3) beta gamma t, counters)"""
        tk, gk, hk, ck = self.oscene(key).intersect(o, d, self.oracle.KD_ORDERED, node_boxes=self.boxes(key), threads=8)
        return tk, gk, np.where(tk[:, None] >= 0, hk[:, :3], 0.0).astype(f32), ck

    def walk_all(self, key):
        if key not in self._walk:
            o, d, _, _ = self.rays(key)
            self._walk[key] = self.walk(key, o, d)
        return self._walk[key]

    def brute_all(self, key):
        name, _, kd = CONFIGS[key]
        if (name, kd) not in self._brute:
            o, d, _, _ = self.rays(key)
            tb, _, hb, _ = self.oscene(key).intersect(o, d, self.oracle.BRUTE, threads=8)
            self._brute[(name, kd)] = tb, np.where(tb[:, None] >= 0, hb[:, :3], 0.0).astype(f32)
        return self._brute[(name, kd)]


@pytest.fixture(scope="module")
def ctx(mcpt, oracle_mod):
    return Ctx(mcpt, oracle_mod)


def assert_visits(st, ck, what=""):
    for k in VISITS:
        assert st[k] == ck[k], (what, k, st[k], ck[k])


def contract_t_max(info, n):
    """the classes FLT_MAX / 8 / 4 of test_gpu_rayquery.py, for D in units of the scaled direction"""
    base = np.array([FLT_MAX, 8.0, 4.0], f32)[np.arange(n) % 3]
    unbounded = base == f32(FLT_MAX)
    scaled = np.ldexp(np.where(unbounded, f32(1), base), -info["scale_exp"]).astype(f32)
    return np.where(unbounded, base, scaled).astype(f32)


# ---- 1. closest hit ------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_closest_hit_in_contract_equals_the_oracle_walk_and_the_brute_force(ctx, key):
    """A-D through trace_device, Scene.intersect and the lean query"""
    scene = ctx.scene(key)
    o_all, d_all, fam, info = ctx.rays(key)
    tk_all, _, hk_all, _ = ctx.walk_all(key)
    tb_all, hb_all = ctx.brute_all(key)
    miss = R.root_box_miss(ctx.oscene(key), o_all, d_all)
    print(key, "rays per family", np.bincount(fam).tolist(),
          "hit fractions", [round(float((tk_all[fam == f] >= 0).mean()), 3) for f in range(5)],
          "root-box misses", [int(miss[fam == f].sum()) for f in range(5)])
    for f in (R.FAM_A, R.FAM_B, R.FAM_C, R.FAM_D):
        m = fam == f
        o, d = ctx.pick(key, m)
        what = (key, R.FAMILY_NAMES[f])
        tk, _, hk, ck = ctx.walk(key, o, d)
        assert np.array_equal(tk, tk_all[m]) and 0.3 < (tk >= 0).mean() < 1.0
        scene.trace_stats()                               # a fresh record
        tri, hit = trace(scene, o, d)
        st = scene.trace_stats()
        assert_same_hits(tri, hit, tk, hk, what)
        assert st["rays"] == o.shape[0]
        assert_visits(st, ck, what)
        rt, rh, rs = scene.intersect(o, d)
        assert_same_hits(rt, rh, tk, hk, what + ("intersect",))
        assert rs["rays"] == o.shape[0]
        assert_visits(rs, ck, what + ("intersect",))
        tri_l, hit_l = trace(scene, o, d, lean=True)
        assert_same_hits(tri_l, hit_l, tk, hk, what + ("lean",))
        # the brute force: every ray but D's copies of rays that start on a triangle edge
        bad = np.nonzero((tri != tb_all[m]) | (_bits(hit) != _bits(hb_all[m])).any(axis=1))[0]
        ex = info["exempt"][m]
        assert ex[bad].all(), (what, bad[~ex[bad]][:10])
        assert bad.size <= 50 and (f == R.FAM_D or bad.size == 0), (what, bad.size)


@pytest.mark.parametrize("key", KEYS)
def test_subnormal_components_get_the_oracle_walk_s_answer_as_given(ctx, key):
    """E, outside the contract: what is returned there is the walk's answer, and the device
    computes it on the subnormal values as they are (no flush to zero): ids, hit bits, counters."""
    scene = ctx.scene(key)
    _, _, fam, _ = ctx.rays(key)
    o, d = ctx.pick(key, fam == R.FAM_E)
    tk, _, hk, ck = ctx.walk(key, o, d)
    assert (tk >= 0).any() and (tk < 0).any()
    scene.trace_stats()
    tri, hit = trace(scene, o, d)
    st = scene.trace_stats()
    assert_same_hits(tri, hit, tk, hk, key)
    assert_visits(st, ck, key)
    rt, rh, rs = scene.intersect(o, d)
    assert_same_hits(rt, rh, tk, hk, (key, "intersect"))
    assert_visits(rs, ck, (key, "intersect"))
    tri_l, hit_l = trace(scene, o, d, lean=True)
    assert_same_hits(tri_l, hit_l, tk, hk, (key, "lean"))
    assert np.array_equal(occluded(scene, o, d), (tk >= 0).astype(np.uint8))


# ---- 2. any hit ------------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_any_hit_is_the_closest_hit_flag_under_per_ray_t_max(ctx, key):
    scene = ctx.scene(key)
    o, d, fam, info = ctx.rays(key)
    n = o.shape[0]
    tm = contract_t_max(info, n)
    tk, _, hk, _ = ctx.walk_all(key)
    scene.trace_stats()
    tri, hit = trace(scene, o, d, tm=tm)
    st_c = scene.trace_stats()
    # strict t < t_max: the closest hit if it lies before t_max, else none (where the walk is
    # the brute force: A-D off the exempt rays)
    held = (fam != R.FAM_E) & ~info["exempt"]
    want = np.where(hk[:, 2] < tm, tk, -1)
    assert np.array_equal(tri[held], want[held])
    assert np.array_equal(_bits(hit[held & (tri >= 0)]), _bits(hk[held & (tri >= 0)]))
    for f in range(5):
        cut = (tk >= 0) & (tri < 0) & (fam == f)
        assert cut.sum() >= 50, (key, f, int(cut.sum()))   # t_max does cut hits off in every family
    occ = occluded(scene, o, d, tm=tm)
    st_a = scene.trace_stats()
    assert np.array_equal(occ, (tri >= 0).astype(np.uint8))
    occ_h, st_h = scene.occluded(o, d, t_max=tm)
    assert np.array_equal(occ_h, occ)
    for st in (st_a, st_h):
        assert st["rays"] == st_c["rays"] == n
        for k in VISITS:
            assert st[k] <= st_c[k], (k, st[k], st_c[k])
    assert_counters(st_h, st_a, "host entry")


@pytest.mark.parametrize("key", KEYS)
def test_nothing_is_occluded_before_a_far_origin_reaches_the_scene(ctx, key):
    """B's origins more than 2.5 from the root box, unit directions, t_max = 2: no hit, no early
    exit -- the any-hit walk is the closest-hit walk and counts like it."""
    scene = ctx.scene(key)
    o, d, fam, _ = ctx.rays(key)
    nodes = ctx.oscene(key).kd_nodes()
    bmin, bmax = nodes[0, 4:7].view(f32), nodes[0, 7:10].view(f32)
    gap = np.linalg.norm(np.maximum(np.maximum(bmin - o, o - bmax), 0).astype(np.float64), axis=1)
    far = (fam == R.FAM_B) & (gap > 2.5)
    assert far.sum() >= 1000 and (ctx.walk_all(key)[0][far] >= 0).sum() >= 300
    o, d = ctx.pick(key, far)
    scene.trace_stats()
    tri, _ = trace(scene, o, d, t_max=2.0)
    st_c = scene.trace_stats()
    occ = occluded(scene, o, d, t_max=2.0)
    st_a = scene.trace_stats()
    assert (tri == -1).all() and not occ.any()
    assert_counters(st_a, st_c, (key, "t_max 2"))
    occ_h, st_h = scene.occluded(o, d, t_max=2.0)
    assert not occ_h.any()
    assert_counters(st_h, st_c, (key, "host t_max 2"))


# ---- 3. batch shapes ---------------------------------------------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene03"])
@pytest.mark.parametrize("n", [1, 63, 65])
def test_batches_whose_waves_all_leave_at_the_root_box(ctx, key, n):
    """A's origins outside the box along a zero axis: every ray misses in begin_ray, a whole
    wave is ready at once and a workgroup refills with no lane ever traversing.  Then the same
    sizes with A's other outside origins mixed in, some of which do traverse."""
    scene = ctx.scene(key)
    _, _, fam, info = ctx.rays(key)
    a = fam == R.FAM_A
    zero_axis = a & (info["sub"] == R.A_OUT_ZERO_AXIS)
    outside = a & (info["sub"] != R.A_INSIDE)
    for name, mask in (("zero axis", zero_axis), ("outside", outside)):
        o, d = ctx.pick(key, mask)
        step = o.shape[0] // n
        o, d = np.ascontiguousarray(o[::step][:n]), np.ascontiguousarray(d[::step][:n])
        assert o.shape[0] == n
        tk, _, hk, ck = ctx.walk(key, o, d)
        if name == "zero axis":
            assert (tk == -1).all() and ck["inner_visits"] == ck["leaf_visits"] == 0
        elif n > 1:
            assert ck["inner_visits"] > 0
        scene.trace_stats()
        tri, hit = trace(scene, o, d)
        st = scene.trace_stats()
        assert_same_hits(tri, hit, tk, hk, (key, n, name))
        assert st["rays"] == n
        assert_visits(st, ck, (key, n, name))
        rt, rh, rs = scene.intersect(o, d)
        assert_same_hits(rt, rh, tk, hk, (key, n, name, "intersect"))
        assert_visits(rs, ck, (key, n, name, "intersect"))
        assert np.array_equal(occluded(scene, o, d), (tk >= 0).astype(np.uint8))
        assert scene.trace_stats()["rays"] == n


@pytest.mark.parametrize("key", ["scene01", "scene03"])
def test_one_workgroup_refills_lane_by_lane_over_signed_zeros_and_outside_origins(ctx, key):
    """workgroups=1, refill=1 on 5000 rays of A and B: nearly half of them leave at the root box"""
    scene = ctx.scene(key)
    o, d, fam, _ = ctx.rays(key)
    idx = np.nonzero((fam == R.FAM_A) | (fam == R.FAM_B))[0]
    idx = idx[np.random.default_rng(3).permutation(idx.size)[:5000]]
    o, d = np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])
    tk, _, hk, ck = ctx.walk(key, o, d)
    assert 0.3 < (tk >= 0).mean() < 0.7
    scene.trace_stats()
    tri, hit = trace(scene, o, d, workgroups=1, refill=1)
    st = scene.trace_stats()
    assert_same_hits(tri, hit, tk, hk, key)
    assert st["rays"] == 5000
    assert_visits(st, ck, key)
    assert np.array_equal(occluded(scene, o, d, workgroups=1, refill=1), (tk >= 0).astype(np.uint8))


# ---- 4. radiance ---------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["scene01", "scene01-global", "scene03"])
def test_depth_zero_radiance_is_the_emission_at_the_oracle_walk_s_hit(ctx, key):
    """A-C (unit directions), max_depth 0: as tests/test_gpu_radiance.py's depth-0 test"""
    scene, osc = ctx.scene(key), ctx.oscene(key)
    _, _, fam, _ = ctx.rays(key)
    o, d = ctx.pick(key, fam <= R.FAM_C)
    n = o.shape[0]
    scene.trace_stats()
    got = radiance(scene, o, d, spp=1, max_depth=0)
    st = scene.trace_stats()
    tri, geom, _, ck = ctx.walk(key, o, d)
    hit = tri >= 0
    ka = osc.geoms()[np.where(hit, geom, 0)][:, 0:3].astype(f32)
    want = np.where(hit[:, None], f32(1) * (ka * f32(10.0)), f32(0)).astype(f32)
    assert same(got, want)
    assert 0.3 < hit.mean() < 1.0 and (want > 0).any()
    assert st["rays"] == n == st["paths"] and st["shades"] == 0
    assert_visits(st, ck, key)


def test_radiance_paths_from_contract_rays_do_not_depend_on_the_layout(ctx):
    """A-C, depth 7, 2 spp: the LDS layout and the child-box records give the same bits"""
    _, _, fam, _ = ctx.rays("scene01")
    o, d = ctx.pick("scene01", fam <= R.FAM_C)
    res = []
    for key in ("scene01", "scene01-global"):
        scene = ctx.scene(key)
        scene.trace_stats()
        res.append((radiance(scene, o, d, spp=2, max_depth=7), scene.trace_stats()))
    (a, sa), (b, sb) = res
    assert same(a, b)
    assert (a > 0).any()
    for k in ("rays", "paths", "shades"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    assert sa["paths"] == 2 * o.shape[0] and sa["shades"] > 0

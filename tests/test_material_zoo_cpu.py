"""The material-ends scenes (tests/_matzoo.py) without a GPU: that the oracle is well
defined on them (its ordered walk, its child-box walk and its brute force give one
image), that they exercise what they are for -- NaN rays made by the path loop itself,
NaN radiance from an overflowed throughput, every class boundary of the scatter -- and
known answers of the oracle's samplers and walks that tell the rule from its neighbouring
wrong forms.  tests/test_gpu_material_zoo.py renders the same scenes on the GPU against
this oracle; these pins are why its comparisons mean something.
"""
import ctypes as C

import numpy as np
import pytest

import _aov_ref as A
import _sampler_grid as G
from _matzoo import (EDGE_MATERIALS, MATZOO, edge_material_of, edges_mtl, edges_obj, matzoo_scenes,  # noqa: F401
                     same_nan_aware)
from _zoo import ZOO_CAM

f32 = np.float32
W = H = 64
SPP, CHUNK = 5, 2
GAIN = ("gain20", "gain18", "gain19")
QE_KW = dict(seed=0x5EED, illum=1.0, fov=45.0, fresnel_kd=0)
QNAN = (0x7FC00000, 0xFFC00000)


@pytest.fixture(scope="module")
def oscenes(oracle_mod, matzoo_scenes):  # noqa: F811
    have = {}

    def get(name):
        if name not in have:
            have[name] = oracle_mod.Scene(matzoo_scenes[name])
        return have[name]

    return get


def _render(oracle_mod, scene, depth, qe=False, **kw):
    if qe:
        kw = dict(QE_KW, mode=oracle_mod.MODE_QE, **kw)
    return scene.render(oracle_mod.RenderParams(width=W, height=H, spp=SPP, spp_chunk=CHUNK, max_depth=depth, threads=16,
                                                **ZOO_CAM, **kw))


# ---- the oracle is one oracle on these scenes -----------------------------------------------

@pytest.mark.parametrize("qe", [False, True], ids=["cv", "qe"])
@pytest.mark.parametrize("name", MATZOO)
def test_oracle_walks_agree(oracle_mod, oscenes, name, qe):
    """ordered walk = child-box walk = brute force, NaN pixels (gain20 only) in the same places"""
    for depth in ((5,) if qe else (1, 2, 3, 7)):
        imgs = [_render(oracle_mod, oscenes(name), depth, qe, traversal=t, node_boxes=b)[0]
                for t, b in ((oracle_mod.KD_ORDERED, 0), (oracle_mod.KD_ORDERED, 1), (oracle_mod.BRUTE, 0))]
        assert np.nanmax(imgs[0]) > 0
        assert same_nan_aware(imgs[0], imgs[1]) and same_nan_aware(imgs[0], imgs[2]), (name, depth)
        if name in ("edges", "nanfloor", "gain18", "gain19"):
            assert np.isfinite(imgs[0]).all(), (name, depth)


def test_every_scene_is_small_and_builds_both_layouts(mcpt, matzoo_scenes):  # noqa: F811
    for name in MATZOO:
        m = mcpt.ObjModel(matzoo_scenes[name])
        assert m.info()["n_triangles"] < 60
        for layout, boxes in (("auto", 0), ("global", 1)):
            assert mcpt.Scene(m, layout=layout, host_only=True).info()["node_boxes"] == boxes


# ---- nanfloor: the path loop makes NaN rays ---------------------------------------------------

def _centre_rays(oracle_mod, cam):
    """the primary rays through the pixel centres (a jitter of zero), as _aov_ref.primary_rays forms them"""
    L = oracle_mod.lib()
    fwd, upv, right = oracle_mod.camera_basis(cam["eye"], cam["direction"], (0.0, 1.0, 0.0))
    ys, xs = np.mgrid[0:H, 0:W]
    th = np.float64(L.orc_tan_half_fov(C.c_float(60.0)))
    idx = ((2.0 * xs.astype(np.float64) / W - 1) * th).astype(f32)
    idy = ((1.0 * H / W - 2.0 * ys.astype(np.float64) / W) * th).astype(f32)
    d = A.normalize_cu(A._rot(right, upv, fwd, idx, idy, f32(-1))).reshape(-1, 3)
    return np.broadcast_to(np.asarray(cam["eye"], f32), d.shape).copy(), np.ascontiguousarray(d)


def test_nanfloor_first_bounce_makes_nan_directions(oracle_mod, oscenes):
    """the first bounce restated: the pixel-centre rays' hits on the floor (Tr 0.9, Ni 0.8, normal
    (0, 1, 0)) through orc_sample_fresnel with the smallest uniform, so every sample transmits.
    Measured: 1228 centres hit the floor first, 658 of them beyond the critical angle"""
    s = oscenes("nanfloor")
    o, d = _centre_rays(oracle_mod, ZOO_CAM)
    tri, geom, _, _ = s.intersect(o, d, oracle_mod.KD_ORDERED)
    g = s.geoms()
    floor = np.flatnonzero((g[:, 10] > 0) & (g[:, 11] == f32(0.8)))
    assert len(floor) == 1
    k = np.flatnonzero((tri >= 0) & (geom == floor[0]))
    n = np.tile(f32([0, 1, 0]), (len(k), 1))
    u = np.tile(f32([G.U_MIN, 0]), (len(k), 1))
    par = np.tile(f32([0.9, 0.8]), (len(k), 1))
    out = G.oracle_outputs(oracle_mod, "fresnel", n, np.ascontiguousarray(d[k]), u, par)
    nan = np.isnan(out).all(axis=1)
    print("floor hits %d, NaN directions %d" % (len(k), int(nan.sum())))
    assert np.array_equal(nan, np.isnan(out).any(axis=1))           # a NaN direction is NaN in every component
    assert len(k) >= 1000 and nan.sum() >= 500
    # beyond the critical angle, and only there: 1 - (1 - c^2) / Ni^2 < 0 with c = -d.y
    c = d[k][:, 1].astype(np.float64)
    assert np.array_equal(nan, 1 - (1 - c * c) / 0.64 < -1e-6) or np.array_equal(nan, 1 - (1 - c * c) / 0.64 < 1e-6)
    # the next origin hp + 0.01 * dir is then NaN too, and the path still ends: the image is finite
    img, cnt = _render(oracle_mod, s, 7)
    assert np.isfinite(img).all() and cnt["rays"] > cnt["paths"]


# ---- NaN rays in the oracle's walks -----------------------------------------------------------

def _nan_walk(scene, origin):
    """The ordered walk's rule for a ray whose direction is NaN, restated on the node table: the plane
    distance t is NaN, so `!(t > 0)` holds and only the near child is entered, nothing pushed; near is
    the left child where origin < split, else the right one (a NaN origin compares false).  Every
    triangle of the one leaf reached is tested, none is hit.  -> (inner visits, leaf refs)"""
    nodes = scene.kd_nodes()
    i, inner = 0, 0
    while nodes[i, 2]:
        inner += 1
        a = int(nodes[i, 2]) - 1
        sv = nodes[i, 3:4].view(f32)[0]
        i = int(nodes[i, 0] if origin[a] < sv else nodes[i, 1])
    return inner, int(nodes[i, 11])


@pytest.mark.parametrize("name", ["edges", "nanfloor"])
def test_oracle_walks_nan_rays_to_one_leaf_and_miss(oracle_mod, oscenes, name):
    """1000 all-NaN rays of either sign bit and 1000 rays with a NaN direction from finite origins:
    both walks miss, and count what the rule above gives -- whatever the NaNs' signs (the kernels
    order slab ends by the direction's sign bit, the oracle by value: neither may matter)"""
    s = oscenes(name)
    n = 1000
    sign = (np.arange(3 * n) % 5 < 2).reshape(n, 3)
    nan = np.where(sign, QNAN[1], QNAN[0]).astype(np.uint32).view(f32)
    lo, hi = s.kd_nodes()[0, 4:7].view(f32), s.kd_nodes()[0, 7:10].view(f32)
    t = ((np.arange(3 * n).reshape(n, 3) * np.array([7, 11, 13])) % 101) / 100.0
    finite = (lo - 1 + t * (hi - lo + 2)).astype(f32)                  # a lattice over the root box and a margin
    for origins in (nan, finite):
        want = [_nan_walk(s, o) for o in origins]
        inner, refs = sum(w[0] for w in want), sum(w[1] for w in want)
        assert inner >= n and refs >= 1
        for d in (nan, (nan.view(np.uint32) ^ np.uint32(0x80000000)).view(f32)):
            for boxes in (0, 1):
                tri, _, _, c = s.intersect(origins, d, oracle_mod.KD_ORDERED, node_boxes=boxes)
                assert (tri == -1).all()
                assert (c["inner_visits"], c["leaf_visits"], c["leaf_refs"], c["tri_tests"]) == (inner, n, refs, refs), boxes
            assert (s.intersect(origins, d, oracle_mod.BRUTE)[0] == -1).all()
    if name == "edges":                                                 # (the all-NaN ray's walk, as measured)
        assert _nan_walk(s, nan[0]) == (4, 2)


# ---- gain scenes: NaN radiance and the host's decision ----------------------------------------

def test_gain20_has_nan_pixels_from_depth_2_on(oracle_mod, oscenes):
    """Kd 1e20: two bounces overflow the throughput, and the terminal query's inf * 0 is NaN.
    Measured: 0 / 269 / 751 / 25 NaN pixels at depths 1 / 2 / 3 / 7"""
    counts = {}
    for depth in (1, 2, 3, 7):
        img = _render(oracle_mod, oscenes("gain20"), depth)[0]
        counts[depth] = int(np.isnan(img).any(axis=2).sum())
    print("gain20 NaN pixels by depth:", counts)
    assert counts[1] == 0 and min(counts[2], counts[3], counts[7]) > 0
    assert np.isfinite(_render(oracle_mod, oscenes("gain20"), 1)[0]).all()


def test_gain_scenes_keep_their_emitter_box_on_the_host(mcpt, matzoo_scenes):  # noqa: F811
    """Kd is finite, so the scene qualifies (host_model.cpp terminal_cull_boxes); whether a render
    may use the box is the render's decision (plan.cpp: the gain rule, by max_depth)"""
    for name in GAIN:
        for layout in ("auto", "global"):
            s = mcpt.Scene(mcpt.ObjModel(matzoo_scenes[name]), layout=layout, host_only=True)
            assert s.info()["terminal_cull_boxes"] == 1, (name, layout)
    assert mcpt.Scene(mcpt.ObjModel(matzoo_scenes["gain19_nocull"]), host_only=True).info()["terminal_cull_boxes"] == 0


def test_gain18_and_gain19_trace_the_same_rays(oracle_mod, oscenes):
    """Kd changes no ray in CVMCTracer mode: what the GPU test compares between the two scenes and
    gain19's twin without emitter boxes are fates of one and the same set of rays"""
    cnts = [_render(oracle_mod, oscenes(n), 7)[1] for n in ("gain18", "gain19", "gain19_nocull")]
    assert cnts[0] == cnts[1] == cnts[2]
    for n in ("gain18", "gain19"):
        assert np.isfinite(_render(oracle_mod, oscenes(n), 7)[0]).all()


# ---- edges: the classes as loaded ---------------------------------------------------------------

def _class(row):
    """trace_device.hpp is_emitter / material_class on a geometry row (Ka, Kd, Ks, Ns, Tr, Ni)"""
    if (row[0:3] > 0).any():
        return 0                                                        # emitter: never scatters
    return 3 if row[10] > 0 else (2 if row[9] > 1 else 1)


def test_edges_geometries_are_loaded_as_written(mcpt, oracle_mod, oscenes, matzoo_scenes):  # noqa: F811
    m = mcpt.ObjModel(matzoo_scenes["edges"])
    s = mcpt.Scene(m, host_only=True)
    geoms = s.kd()[3]
    assert np.array_equal(geoms.view(np.uint32), oscenes("edges").geoms().view(np.uint32))
    names = sorted(k for k, t in m.groups().items() if len(t))          # geometries: the groups in name order
    assert len(names) == len(geoms)
    mat = edge_material_of()

    def row(obj):
        return geoms[names.index(obj if obj in names else obj + "_0")]

    by_mat = {mat[o]: row(o) for o in mat}
    assert set(by_mat) == {n for n, _ in EDGE_MATERIALS}                 # every material is on some object
    ns = {k: by_mat[k][9] for k in by_mat}
    assert ns["ns1"] == 1 and ns["ns1_5"] == f32(1.5) and ns["ns2_7"] == f32(2.7) and ns["ns1e6"] == f32(1e6)
    assert ns["ns5e9"] == f32(5e9) and ns["ns5e9"] >= f32(4294967040.0)  # scene_image.cpp: Ns_u = 0xFFFFFF00
    assert ns["ns_default"] == 2 and ns["kd2"] == 1                      # a Ks line alone: Ns 2; no Ks: Ns 1
    assert [_class(by_mat[k]) for k in ("ns1", "ns1_5", "ns_default", "ns5e9", "kd2")] == [1, 2, 2, 2, 1]
    assert [_class(by_mat[k]) for k in ("ni1", "ni0_8", "tr2", "tr0_001", "glowglass")] == [3, 3, 3, 3, 0]
    assert by_mat["glowglass"][10] > 0                                   # glass by Tr, yet an emitter
    assert by_mat["kd2"][3] == 2 and tuple(by_mat["ks_rgb"][6:9]) == (f32(0.9), f32(0.5), f32(0.2))
    assert (by_mat["tr2"][10], by_mat["ni3"][11], by_mat["ni0_8"][11]) == (2, 3, f32(0.8))


def _edges_variant(oracle_mod, tmp_path, tag, **override):
    d = tmp_path / tag
    d.mkdir()
    (d / "edges.obj").write_text(edges_obj())
    (d / "edges.mtl").write_text(edges_mtl(**override))
    return oracle_mod.Scene(str(d / "edges.obj"))


def test_edges_class_boundaries_in_the_path_loop(oracle_mod, oscenes, tmp_path):
    """Whole renders that move one material across a boundary and must, or must not, change:
    CV Phong takes (unsigned)Ns, so Ns 2.7 renders as Ns 2 and Ns 1.5 as Ns 1.99 -- QE Phong takes
    the float, and differs; Ns exactly 1 is diffuse, so its Ks line is dead -- were it Phong
    (`Ns >= 1`) the Ks would tint it"""
    base = {qe: _render(oracle_mod, oscenes("edges"), 3, qe)[0] for qe in (False, True)}
    trunc = _edges_variant(oracle_mod, tmp_path, "trunc", ns2_7="Kd 0.1 0.1 0.1\nKs 0.9 0.9 0.9\nNs 2",
                           ns1_5="Kd 0.1 0.1 0.1\nKs 0.9 0.9 0.9\nNs 1.99")
    assert np.array_equal(_render(oracle_mod, trunc, 3)[0].view(np.uint32), base[False].view(np.uint32))
    assert not np.array_equal(_render(oracle_mod, trunc, 3, True)[0].view(np.uint32), base[True].view(np.uint32))
    for tag, lines in (("noks", "Kd 0.6 0.6 0.2"), ("ks0", "Kd 0.6 0.6 0.2\nKs 0 0 0\nNs 1")):
        v = _edges_variant(oracle_mod, tmp_path, tag, ns1=lines)
        for qe in (False, True):
            assert np.array_equal(_render(oracle_mod, v, 3, qe)[0].view(np.uint32), base[qe].view(np.uint32)), (tag, qe)
    # and the boundary is a boundary: just above 1 the material is Phong and the image moves
    above = _edges_variant(oracle_mod, tmp_path, "above", ns1="Kd 0.6 0.6 0.2\nKs 1 1 1\nNs 1.0000001")
    assert not np.array_equal(_render(oracle_mod, above, 3)[0].view(np.uint32), base[False].view(np.uint32))


# ---- known answers of the samplers --------------------------------------------------------------

def _one(oracle_mod, op, n, d, u, par):
    return G.oracle_outputs(oracle_mod, op, f32([n]), f32([d]), f32([u]), f32([par]))[0]


def test_entering_beyond_the_critical_angle_is_nan_not_a_mirror(oracle_mod):
    """Ni 0.8, 60 degrees off the normal, arriving from outside: 1 - (1 - 0.25) / 0.64 < 0.  The
    reference applies its total-internal-reflection test to leaving rays only"""
    n, d = f32([0, 1, 0]), G.incident(f32([0, 1, 0]), 0.5, -1)
    for op in ("fresnel", "fresnel_qe"):
        assert np.isnan(_one(oracle_mod, op, n, d, (G.U_MIN, 0), (0.9, 0.8))).all()
        # the same ray leaving (Ni 1.5 beyond its critical angle) is the mirror direction, finite
        out = _one(oracle_mod, op, n, -d, (G.U_MIN, 0), (0.9, 1.5))
        mirror = (-d) - 2 * np.dot(-d, n) * n
        assert np.allclose(out, mirror, atol=1e-6)
        # and inside the critical angle entering refracts: finite, through the surface
        out = _one(oracle_mod, op, n, G.incident(n, 0.9, -1), (G.U_MIN, 0), (0.9, 0.8))
        assert np.isfinite(out).all() and out[1] < 0


def test_fresnel_decision_is_strict_and_tr_2_always_transmits(oracle_mod):
    """x < Tr * F transmits; x == Tr * F reflects.  Tr 2 at normal incidence: Tr * F = 2 > every uniform"""
    n = f32([0, 1, 0])
    cases = 0
    for cos in (1.0, 0.8, 0.3):
        d = G.incident(n, cos, -1)
        for tr in (0.5, 0.9):
            t = G.tr_f(n, d, tr)
            assert 0 < t < 1
            at = _one(oracle_mod, "fresnel", n, d, (t, 0), (tr, 1.5))
            below = _one(oracle_mod, "fresnel", n, d, (np.nextafter(t, f32(0)), 0), (tr, 1.5))
            assert at[1] > 0 and below[1] < 0, (cos, tr, at, below)      # reflected up / refracted down
            cases += 1
    assert cases == 6
    for x in (G.U_MIN, f32(0.5), G.U_BELOW_1, f32(1.0)):
        assert _one(oracle_mod, "fresnel", n, G.incident(n, 1.0, -1), (x, 0), (2.0, 1.5))[1] < 0
    # Tr 1 does not: at x = 1.0f (rng_next's largest value) nothing is below Tr * F <= 1
    assert _one(oracle_mod, "fresnel", n, G.incident(n, 1.0, -1), (1.0, 0), (1.0, 1.5))[1] > 0


def test_cv_phong_truncates_ns_where_qe_phong_does_not(oracle_mod):
    n, d, u = f32([0, 1, 0]), G.incident(f32([0, 1, 0]), 0.6, -1), (0.25, 0.7)
    cv2 = _one(oracle_mod, "phong", n, d, u, (np.array([2], np.uint32).view(f32)[0], 0))
    qe2, qe27 = (_one(oracle_mod, "phong_qe", n, d, u, (v, 0)) for v in (2.0, 2.7))
    assert np.array_equal(cv2.view(np.uint32), qe2.view(np.uint32))
    assert not np.array_equal(cv2.view(np.uint32), qe27.view(np.uint32))


def test_unsigned_ns_saturates_below_2_to_the_32(oracle_mod):
    """CV Phong's (unsigned)Ns as the scene image stores it (scene_image.cpp Ns_u): truncation, and
    from the largest float below 2^32 on that value -- C leaves the plain conversion undefined there
    (x86 wrapped 5e9 to 705032704, another exponent than the kernels')"""
    L = oracle_mod.lib()
    top = f32(4294967040.0)
    for ns, want in ((0.0, 0), (-3.0, 0), (0.5, 0), (1.5, 1), (2.7, 2), (1e6, 10 ** 6), (np.nextafter(top, f32(0)), 0xFFFFFE00),
                     (top, 0xFFFFFF00), (5e9, 0xFFFFFF00), (np.inf, 0xFFFFFF00)):
        assert L.orc_ns_u(float(ns)) == want, ns
    assert f32(np.uint32(0xFFFFFF00 + 1)) == top                        # ns1 = (float)(Ns_u + 1u): no wrap to 0


def test_the_sampler_grid_reaches_every_branch(oracle_mod):
    """what tests/test_gpu_math.py's grid sends through the device samplers, by the oracle's outputs"""
    nrm, din, u, par = G.fresnel_cases()
    out = G.oracle_outputs(oracle_mod, "fresnel", nrm, din, u, par)
    ndoti = np.einsum("ij,ij->i", nrm.astype(np.float64), din.astype(np.float64))
    nan = np.isnan(out).any(axis=1)
    through = np.einsum("ij,ij->i", out.astype(np.float64), nrm.astype(np.float64)) * ndoti > 0
    assert nan.sum() >= 100 and (ndoti[nan] < 0).all() and (par[nan, 1] < 1).all()
    for side in (ndoti < 0, ndoti > 0):
        assert (through & side & ~nan).sum() >= 500 and (~through & side & ~nan).sum() >= 500
    tir = (ndoti > 0) & (1 - (1 - ndoti * ndoti) * par[:, 1].astype(np.float64) ** 2 < -1e-9) & (u[:, 0] == G.U_MIN)
    assert tir.sum() >= 50 and not through[tir].any()
    assert 2000 <= len(nrm) <= 20000
    nrm, _, _, _ = G.lobe_cases(None)
    ny = nrm[:, 1]
    eps = f32(1.192092896e-07)
    assert (np.abs(ny + 1) < eps).any() and (np.abs(ny - 1) < eps).any()
    general = (np.abs(ny + 1) >= eps) & (np.abs(ny - 1) >= eps)
    assert (general & (np.abs(ny) > 0.999999)).any() and (general & (ny == 0)).any()

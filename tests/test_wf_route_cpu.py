"""A wavefront render's route and batch split (csrc/wf_route.hpp) without a GPU.

tests/cpp/wf_route_probe.cpp prints wf_route over a grid of scene and render
facts -- lean, wf_sort, mode, listed, tile 8 / 4, default batch, occluder
boxes, direct lists, emitter boxes, kListMaxTris and one more triangle, five
images (small; the largest beside which the direct lists fit and 16 B more; a
small and a large one built for global memory), the largest material table that
fits beside the extend and one geometry more -- then the routes the GPU suite
pins by counters, then the batch split of small frames.  The tests assert what
must follow from what, not a second copy of the rule.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(words):
    return {k: int(v) for k, v in (w.split("=") for w in words)}


@pytest.fixture(scope="module")
def probe():
    sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
    import build_dropin
    out = subprocess.run([build_dropin.build("wf_route_probe")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    consts, rows, named, splits = {}, [], {}, []
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "B":
            splits[-1][1].append(tuple(map(int, w[1:])))
        elif w[0] == "R":
            rows.append(_fields(w[1:]))
        elif w[0] == "S":
            splits.append((_fields(w[1:]), []))
        elif w[0] == "N":
            named[w[1]] = _fields(w[2:])
        elif w[0] == "C":
            consts.update(_fields(w[1:]))
    return consts, rows, named, splits


def test_grid_is_the_one_described(probe):
    c, rows, _, _ = probe
    assert len(rows) == 5 * 2 ** 10 * 2
    for key, n in dict(lean=2, sort=2, qe=2, listed=2, tile=2, default_batch=2, n_miss=2, counts=2, n_cull=2,
                       n_tris=2, image=4, node_boxes=2).items():
        assert len({r[key] for r in rows}) == n, key
    assert {r["image"] for r in rows if not r["node_boxes"]} >= {c["fit"], c["fit"] + 16}
    # the two limiting sizes, from the constants: one 16-B unit more no longer fits beside the image
    need = c["stack4"] + c["kLdsCounterBytes"] + c["kShadeStaticLds"] + c["kDirectLdsBytes"]
    assert c["fit"] + need <= c["kMaxLds"] < c["fit"] + 16 + need


def test_route_implications(probe):
    c, rows, _, _ = probe
    cu = c["kLdsPerCu"]
    for r in rows:
        # bounce 0: each form needs the one before it
        if r["primary_shade"]:
            assert r["can_list"] and r["shade_cull"], r
        if r["can_list"]:
            assert r["packet"] and r["lean"] and r["tile"] == 8 and r["n_tris"] <= c["kListMaxTris"], r
        if r["packet"]:
            assert r["in_lds"] and not r["qe"] and not r["listed"], r
        assert r["packet"] or r["generate"], r
        if r["whole"]:
            assert r["can_list"] and r["default_batch"], r
        # the shade's two facts
        assert r["carry"] == (r["shade_cull"] and r["direct"]), r
        assert r["direct"] == (r["r_counts"] != 0), r
        if r["direct"]:
            assert r["in_lds"] and r["r_miss"] and r["r_counts"] == r["counts"], r
        if r["shade_cull"]:
            assert r["in_lds"] and r["r_miss"] and not r["sort"], r
        # a counting render walks every ray
        if not r["lean"]:
            assert not (r["r_miss"] or r["direct"] or r["can_list"] or r["shade_cull"] or r["primary_shade"]), r
            assert r["cull_bounce"] == -1, r
        # the terminal cull: never twice, and once where there is one to run
        assert r["terminal"] == r["queries"] - 1 and r["cull_bounce"] in (-1, r["terminal"]), r
        assert not (r["shade_cull"] and r["cull_bounce"] >= 0), r
        if r["lean"] and (r["qe"] or r["n_cull"]):
            assert r["shade_cull"] != (r["cull_bounce"] == r["terminal"]), r
        if r["lean"] and not r["qe"] and not r["n_cull"]:
            assert r["cull_bounce"] == -1, r
        # where the scene lives
        if r["node_boxes"]:
            assert not r["in_lds"] and r["variant"] == 5 and r["nseg"] == r["cus"] * c["kWfGlobalSegsPerCu"], r
            assert r["xcd_deal"] == 1 and r["group_shift"] == 12, r
            assert (r["shade_block1"], r["shade_block2"]) == (256, 256), r
        else:
            assert r["in_lds"] and r["variant"] == 4 and r["nseg"] == r["cus"], r
            assert r["xcd_deal"] == 0 and r["group_shift"] == 6, r
            assert r["shade_block1"] == 1024 and r["shade_block2"] < 1024, r
        # LDS: what runs together on a CU fits there
        ext_cu = r["extend_lds"] * (1 if r["in_lds"] else c["kWfGlobalSegsPerCu"])
        assert ext_cu <= cu, r
        assert r["direct_lds"] == (c["kDirectLdsBytes"] if r["direct"] else 0), r
        if r["in_lds"]:
            assert r["extend_lds"] == r["packet_lds"] + r["direct_lds"] <= cu, r
            assert r["packet_lds"] == c["stack4"] + r["image"] + c["kLdsCounterBytes"], r
            assert r["primary_shade_lds"] == r["extend_lds"], r
        else:
            assert r["extend_lds"] == c["global_lds"] and not r["primary_shade_lds"], r
        if r["direct"]:
            assert ext_cu + c["kShadeStaticLds"] <= cu, r
        assert r["geo_lds"] in (0, 64 * r["n_geoms"]), r
        if r["geo_lds"]:
            assert ext_cu + c["kShadeStaticLds"] + r["geo_lds"] <= cu, r
        assert bool(r["geo_lds"]) == (r["n_geoms"] <= r["geo_limit"]), r


def test_direct_lists_never_move_the_scene(probe):
    """16 B past direct_lists_fit: the scene stays in LDS, the shade still culls, no ray is direct"""
    c, rows, _, _ = probe
    want = [r for r in rows if r["lean"] and r["n_miss"] and r["counts"] and not r["node_boxes"]]
    at = [r for r in want if r["image"] == c["fit"]]
    past = [r for r in want if r["image"] == c["fit"] + 16]
    assert at and len(at) == len(past)
    for a, p in zip(at, past):
        assert a["direct"] and not p["direct"] and p["in_lds"] and not p["carry"]
        for key in ("shade_cull", "packet", "can_list", "primary_shade", "cull_bounce", "nseg"):
            assert a[key] == p[key], key
    assert any(a["carry"] for a in at)


def test_routes_the_gpu_suite_pins(probe):
    """scene01-sized LDS scene, 64 x 64, 3 spp in chunks of 2 (test_primary_shade, test_gpu_adaptive_wf)"""
    _, _, n, _ = probe
    d = n["default"]
    assert d["fused"] and d["lists"] and d["carry"] and d["direct"] and d["cull_bounce"] == -1 and not d["generate"]
    for name in ("sorted", "tile4", "batch200"):
        assert not n[name]["fused"], name
    assert n["sorted"]["lists"] and n["sorted"]["cull_bounce"] == n["sorted"]["terminal"] and not n["sorted"]["carry"]
    assert not n["tile4"]["can_list"] and n["tile4"]["packet"]
    assert n["batch200"]["can_list"] and not n["batch200"]["whole"] and not n["batch200"]["lists"]
    assert not n["qe"]["packet"] and n["qe"]["generate"] and n["qe"]["queries"] == 3 * n["qe"]["max_depth"] + 1
    assert not n["listed"]["packet"] and not n["listed"]["can_list"] and n["listed"]["generate"]
    assert n["listed"]["carry"] and n["listed"]["shade_cull"]      # (a listed pass keeps the shade's route)
    c = n["counting"]
    assert c["packet"] and not (c["can_list"] or c["r_miss"] or c["direct"] or c["shade_cull"]) and c["cull_bounce"] == -1


def test_batch_split(probe):
    c, _, _, splits = probe
    nseg, gs = c["split_nseg"], c["split_group_shift"]
    assert len(splits) > 300
    for s, batches in splits:
        cover = np.zeros((s["spp"], s["npix"]), dtype=np.int32)
        any_whole = False
        for chunk_index, s_begin, nsc, ns, v0, nb, seg, nb_max in batches:
            assert s_begin == chunk_index * s["chunk"] and ns % nsc == 0 and nsc <= s["chunk"], (s, v0)
            assert 0 < nb <= nb_max and nb * ns <= s["capacity"], (s, v0)
            cover[s_begin:s_begin + ns, v0:v0 + nb] += 1
            assert s_begin + ns <= s["spp"] and v0 + nb <= s["npix"], (s, v0)
            # the fewest whole groups per segment that hold the batch's groups
            groups = -(-nb * ns // (1 << gs))
            assert seg % (1 << gs) == 0 and ((seg >> gs) - 1) * nseg < groups <= (seg >> gs) * nseg, (s, v0)
            if s["whole"] and 64 <= nb_max < s["npix"]:
                assert nb_max % 64 == 0, (s, v0)
            any_whole |= v0 % 64 == 0 and nb % 64 == 0
        assert (cover == 1).all(), s       # every (pixel, sample) in exactly one batch
        assert any_whole == bool(s["any_whole"]), s

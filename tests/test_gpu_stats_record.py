"""The contract of a scene's stats record (include/mcpt.h: mcpt_render_stats_read, the five
route counters, mcpt_scene_primary_tile_classes, mcpt_trace_stats_read), whatever the layout
of the device blocks behind it: a read returns everything counted since the last read and
clears it; renders between two reads add up; the tile classes belong to the last render, not
to a read; what a scene rendered before does not show in its next record; a multi-device
scene's record is the sum over its replicas, each rendering from its own copy of the route
tables; and the ray queries count into blocks of their own, device entries and host entries
apart, beside the render record.

scene01 at 64 x 64, tiles of 8 (64 tiles), 4 samples per pixel in chunks of 2, max_depth 3:
small, and deep enough that rays are clipped and some lose their walk to a sphere (asserted).
"""
import numpy as np
import pytest

from test_gpu_multidevice import devices  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

W = H = 64
COUNTERS = ("rays", "paths", "inner_visits", "leaf_visits", "leaf_refs", "tri_tests", "shades", "stack_spills")
ROUTES = ("direct_rays", "extend_rays", "clipped_rays", "primary_shaded", "sphere_skips")
INTEGERS = COUNTERS + ("renders",) + ROUTES


def _p(mcpt, **kw):
    kw = dict(dict(width=W, height=H, spp=4, spp_chunk=2, tile=8, max_depth=3, pipeline="wavefront", lean=True), **kw)
    return mcpt.RenderParams(**kw)


def _scene(mcpt):
    return mcpt.Scene(mcpt.ObjModel(mcpt.scene_path("scene01")))


def _ints(st, keys=INTEGERS):
    return {k: int(st[k]) for k in keys}


def _classes(scene):
    c = scene.primary_tile_classes()
    return (c["empty"], c["listed"], c["walked"])


def _render_device(scene, p):
    import torch
    fb = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    scene.render_device(p, fb.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return fb.view(H, W, 4)[..., :3].cpu().numpy()


@pytest.fixture(scope="module")
def single(mcpt):
    """the lean wavefront render of a fresh one-device scene: (image, its record), read-only"""
    img, st = _scene(mcpt).render(_p(mcpt))
    img.setflags(write=False)
    print("single:", _ints(st))
    # the frame takes every route the record counts: no assertion below can pass on zeros
    assert st["renders"] == 1 and st["paths"] == W * H * 4 and st["primary_shaded"] == st["paths"]
    assert st["direct_rays"] > 0 and 0 < st["sphere_skips"] < st["clipped_rays"] < st["extend_rays"]
    return img, st


def test_a_read_returns_the_record_and_clears_it(mcpt, single):
    scene = _scene(mcpt)
    img = _render_device(scene, _p(mcpt))
    assert np.array_equal(img, single[0])
    before = _classes(scene)
    assert sum(before) == 64
    first = scene.stats()
    assert _ints(first) == _ints(single[1])
    second = scene.stats()
    assert _ints(second) == dict.fromkeys(INTEGERS, 0)
    assert _classes(scene) == before


def test_renders_between_two_reads_add_up(mcpt, single):
    scene = _scene(mcpt)
    for _ in range(2):
        assert np.array_equal(_render_device(scene, _p(mcpt)), single[0])
    two = _ints(scene.stats())
    assert two == {k: 2 * v for k, v in _ints(single[1]).items()}
    assert two["clipped_rays"] > 0 and two["sphere_skips"] > 0


def test_what_a_scene_rendered_before_does_not_show(mcpt, single):
    a, b = _scene(mcpt), _scene(mcpt)
    # a: the megakernel, then the sorting shade -- no render of it has clipped a walk to a sphere yet
    _, st = a.render(_p(mcpt, pipeline="megakernel"))
    assert _ints(st, ROUTES) == dict.fromkeys(ROUTES, 0)
    _, st = a.render(_p(mcpt, wf_sort=True))
    assert st["clipped_rays"] > 0 and st["sphere_skips"] == 0
    img_a, st_a = a.render(_p(mcpt))
    ca = _classes(a)
    img_b, st_b = b.render(_p(mcpt))
    assert np.array_equal(img_a, img_b) and np.array_equal(img_a, single[0])
    assert _ints(st_a) == _ints(st_b) == _ints(single[1])
    assert ca == _classes(b) and sum(ca) == 64
    img, st = a.render(_p(mcpt, pipeline="megakernel"))
    assert np.array_equal(img, single[0])
    assert _classes(a) == (0, 0, 0) and _ints(st, ROUTES) == dict.fromkeys(ROUTES, 0)
    assert st["rays"] == single[1]["rays"]


def test_replicas_count_as_one_device_does(mcpt, devices, single):  # noqa: F811
    devices([0, 0])
    multi = _scene(mcpt)
    assert multi.info()["n_devices"] == 2
    img, st = multi.render(_p(mcpt))
    assert st["devices"] == 2
    assert np.array_equal(img.view(np.uint32), single[0].view(np.uint32))
    assert _ints(st, ROUTES) == _ints(single[1], ROUTES)
    assert st["rays"] == single[1]["rays"] and st["paths"] == single[1]["paths"]
    assert _ints(multi.stats()) == dict.fromkeys(INTEGERS, 0)


def test_ray_queries_count_beside_the_render_record(mcpt, single):
    import torch
    scene = _scene(mcpt)
    rng = np.random.default_rng(7)
    n = 300
    o = np.tile(np.float32([0.0, 5.0, 15.0]), (n, 1))   # (any origin: the test compares counts with counts)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tri = torch.zeros(n, dtype=torch.int32, device="cuda")

    def device_query():
        scene.trace_device(n, d_o.data_ptr(), d_d.data_ptr(), tri.data_ptr(), lean=False)
        torch.cuda.synchronize()

    _render_device(scene, _p(mcpt))            # a render record waits to be read throughout
    device_query()
    alone = _ints(scene.trace_stats(), COUNTERS)
    assert alone["rays"] == n and alone["inner_visits"] > 0
    assert _ints(scene.trace_stats(), COUNTERS) == dict.fromkeys(COUNTERS, 0)
    device_query()
    m = 100
    _, host = scene.occluded(o[:m], d[:m], lean=False)
    assert host["rays"] == m and host["inner_visits"] > 0
    _, _, host2 = scene.intersect(o[:m], d[:m])
    assert host2["rays"] == m
    # the device entries' block holds the device call alone, the host entry's call its own
    assert _ints(scene.trace_stats(), COUNTERS) == alone
    _, again = scene.occluded(o[:m], d[:m], lean=False)
    assert _ints(again, COUNTERS) == _ints(host, COUNTERS)
    assert _ints(scene.stats()) == _ints(single[1])
    assert _ints(scene.trace_stats(), COUNTERS) == dict.fromkeys(COUNTERS, 0)

"""Host-side mirror of the reference tracer interface, over the C ABI.

Reference interface (pw1316/MonteCarloPathTracer, CVMCTracer/CVMCTracer):
  PW::FileReader::ObjModel::readObj(path)        Framework/ObjReader.hpp:55
  PW::Tracer::Initialize()                       CUDA/CUTracer.h:9
  PW::Tracer::CreateGeometry(const ObjModel*)    CUDA/CUTracer.h:10
  PW::Tracer::DestroyGeometry()                  CUDA/CUTracer.h:11
  PW::Tracer::RenderScene(sceneID, hostcolor)    CUDA/CUTracer.h:12
and its only caller, main.cpp:16-18 / 33-35.

Same names, argument meaning and call order.  Differences:
  * errors raise McptError instead of returning a mostly-ignored cudaError_t;
  * the scene is held by a Tracer object (module functions keep one default
    Tracer, like the reference's module globals);
  * RenderScene keeps the reference's progressive loop (NUM_KERNELS launches of
    NUM_SAMPLES_PER_KERNEL samples, running mean with prevCount, CUTracer.cu:
    378-398) but without the OpenCV window/PNG side effects.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _capi
from ._capi import McptError, RenderParamsC, RenderStats, check, lib

# CV/stdafx.h:41-46
IMG_WIDTH = 800
IMG_HEIGHT = 600
NUM_KERNELS = 100
NUM_SAMPLES_PER_KERNEL = 100
ILLUM = 10.0
DEFAULT_SEED = 0x4D435054


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class ObjModel:
    """PW::FileReader::ObjModel (ObjReader.hpp:37-63): OBJ/MTL data with dummy index 0."""

    FLAVORS = {"cvmctracer": _capi.OBJ_CVMCTRACER, "tinyobj": _capi.OBJ_TINYOBJ}

    def __init__(self, path: Optional[str] = None, flavor: str = "cvmctracer"):
        """flavor "tinyobj": read as QuinEngine does through tinyobjloader
        (mcpt_model_read_obj_ex, include/mcpt.h) -- use it for qe_scene01."""
        self._h = None
        self.path = None
        if path is not None:
            self.read_obj(path, flavor)

    def read_obj(self, path: str, flavor: str = "cvmctracer") -> bool:   # ObjModel::readObj (ObjReader.cpp:8)
        if flavor not in self.FLAVORS:
            raise ValueError(f"flavor must be one of {sorted(self.FLAVORS)}")
        h = C.c_void_p()
        check(lib().mcpt_model_read_obj_ex(path.encode(), self.FLAVORS[flavor], C.byref(h)))
        self._free()
        self._h = h
        self.path = path
        return True

    readObj = read_obj

    @classmethod
    def from_arrays(cls, vertices, normals, triangles, materials, groups: dict) -> "ObjModel":
        """Build from in-memory arrays laid out like ObjReader.hpp:57-63 (element 0 = dummy):
        vertices (n,3), normals (n,3), triangles (n,10) v/t/n/material, materials (n,12)
        Ka Kd Ks Ns Tr Ni, groups {name: triangle indices}."""
        v = np.ascontiguousarray(vertices, np.float32)
        n = np.ascontiguousarray(normals, np.float32)
        t = np.ascontiguousarray(triangles, np.int32)
        m = np.ascontiguousarray(materials, np.float64)
        names = list(groups)
        offs = np.zeros(len(names) + 1, np.int64)
        for i, k in enumerate(names):
            offs[i + 1] = offs[i] + len(groups[k])
        gt = np.ascontiguousarray(np.concatenate([np.asarray(groups[k], np.int32) for k in names])
                                  if names else np.zeros(0, np.int32), np.int32)
        cnames = (C.c_char_p * max(len(names), 1))(*[k.encode() for k in names])
        d = _capi.ModelDesc()
        d.vertices, d.n_vertices = v.ctypes.data_as(C.POINTER(C.c_float)), v.shape[0]
        d.normals, d.n_normals = n.ctypes.data_as(C.POINTER(C.c_float)), n.shape[0]
        d.triangles, d.n_triangles = t.ctypes.data_as(C.POINTER(C.c_int32)), t.shape[0]
        d.materials, d.n_materials = m.ctypes.data_as(C.POINTER(C.c_double)), m.shape[0]
        d.group_names, d.group_offsets = cnames, offs.ctypes.data_as(C.POINTER(C.c_int64))
        d.group_tris, d.n_groups = gt.ctypes.data_as(C.POINTER(C.c_int32)), len(names)
        h = C.c_void_p()
        check(lib().mcpt_model_create(C.byref(d), C.byref(h)))
        obj = cls()
        obj._h = h
        obj.path = "<memory>"
        return obj

    def _free(self):
        if self._h is not None and _capi._lib is not None:
            _capi._lib.mcpt_model_free(self._h)
        self._h = None

    def __del__(self):
        self._free()

    @property
    def handle(self):
        if self._h is None:
            raise McptError(-1, "model not loaded")
        return self._h

    def info(self) -> dict:
        i = _capi.ModelInfo()
        check(lib().mcpt_model_get_info(self.handle, C.byref(i)))
        return {n: int(getattr(i, n)) for n, _ in i._fields_}

    def vertices(self) -> np.ndarray:
        a = np.zeros((self.info()["n_vertices"], 3), np.float32)
        check(lib().mcpt_model_copy_vertices(self.handle, _fptr(a)))
        return a

    def normals(self) -> np.ndarray:
        a = np.zeros((self.info()["n_normals"], 3), np.float32)
        check(lib().mcpt_model_copy_normals(self.handle, _fptr(a)))
        return a

    def triangles(self) -> np.ndarray:
        """(n, 10) int32: vertex[3], texture[3], normal[3], material index."""
        a = np.zeros((self.info()["n_triangles"], 10), np.int32)
        check(lib().mcpt_model_copy_triangles(self.handle, a.ctypes.data_as(C.POINTER(C.c_int32))))
        return a

    def materials(self) -> np.ndarray:
        """(n, 12) float64: Ka[3] Kd[3] Ks[3] Ns Tr Ni."""
        a = np.zeros((self.info()["n_materials"], 12), np.float64)
        check(lib().mcpt_model_copy_materials(self.handle, a.ctypes.data_as(C.POINTER(C.c_double))))
        return a

    def groups(self) -> dict:
        out = {}
        buf = C.create_string_buffer(1024)
        for g in range(self.info()["n_groups"]):
            n = C.c_int64()
            check(lib().mcpt_model_group(self.handle, g, buf, 1024, C.byref(n), None))
            a = np.zeros(n.value, np.int32)
            check(lib().mcpt_model_group(self.handle, g, buf, 1024, C.byref(n),
                                         a.ctypes.data_as(C.POINTER(C.c_int32))))
            out[buf.value.decode()] = a
        return out


PIPELINES = {"megakernel": _capi.PIPELINE_MEGAKERNEL, "wavefront": _capi.PIPELINE_WAVEFRONT}
MODES = {"cvmctracer": _capi.MODE_CVMCTRACER, "quinengine": _capi.MODE_QUINENGINE}
GATHERS = {"peer": _capi.GATHER_PEER, "rccl": _capi.GATHER_RCCL}


@dataclass
class RenderParams:
    """Render configuration; defaults are the CVMCTracer constants for scene 1."""
    width: int = IMG_WIDTH
    height: int = IMG_HEIGHT
    spp: int = NUM_SAMPLES_PER_KERNEL
    spp_offset: int = 0
    spp_chunk: int = 32               # summation chunk (part of the result definition)
    max_depth: int = 7                # CUTracer.cu:212
    illum: float = ILLUM
    fov_deg: float = 60.0             # CUTracer.cu:189
    eye: Sequence[float] = (0.0, 5.0, 17.0)
    direction: Sequence[float] = (0.0, 0.0, -1.0)
    up: Sequence[float] = (0.0, 1.0, 0.0)
    seed: int = DEFAULT_SEED
    prev_count: int = 0
    fresnel_kd: bool = True
    tile: int = 8
    shard_count: int = 1
    shard_index: int = 0
    packed: bool = False
    pipeline: str = "megakernel"      # or "wavefront" (C5): identical image, different kernels
    wf_batch: int = 0                 # wavefront paths per batch and stream, 0 = automatic (include/mcpt.h)
    mode: str = "cvmctracer"          # or "quinengine": rtx.hlsl path semantics (see for_quinengine)
    lean: bool = False                # kernels without traversal counters (same image; bench timing)
    wf_sort: bool = False             # wavefront: shade sorts each block of slots by material; same image
    # scheduling (include/mcpt.h): never changes the image or the counters; 0 = automatic
    wf_streams: int = 0               # wavefront HIP streams (1..4)
    wf_refill: int = 0                # wavefront extend: ready lanes before a wave refills
    wf_group_shift: int = 0           # wavefront, global-memory scenes: 2^k paths per segment group
    ready_thresh: int = 0             # megakernel: ready lanes before a shading round
    tail_units_per_lane: int = 0      # megakernel tail split per lane (< 0: off)
    tail_units: int = 0               # megakernel: exact tail-split units (> 0 overrides)
    wf_mem_limit: int = 0             # wavefront queue memory budget in bytes (0: 90% of free)
    force_peer_copy: bool = False     # multi-device: hipMemcpyPeerAsync also between same-device replicas
    gather: str = "peer"              # multi-device shards to devices[0]: "peer" copies or "rccl" (ncclGather)

    @staticmethod
    def for_scene(scene_id: int, **kw) -> "RenderParams":
        """Camera of RenderScene(sceneID) (CUTracer.cu:347-374)."""
        eye = (0.0, 5.0, 17.0) if scene_id == 1 else (0.0, 5.0, 23.0)
        return RenderParams(eye=eye, **kw)

    @staticmethod
    def for_quinengine(**kw) -> "RenderParams":
        """QuinEngine viewer frame (GraphicsRTX.cpp:163-193, rtx.hlsl:373-404): 1 spp,
        depth 5 with Russian roulette, vertical FOV 45, no ILLUM / Fresnel Kd,
        gamma-2.2 running mean; `seed` is the 32-bit frame seed."""
        base = dict(width=640, height=480, spp=1, spp_chunk=1, max_depth=5, illum=1.0, fov_deg=45.0,
                    fresnel_kd=False, seed=0, mode="quinengine")
        base.update(kw)
        return RenderParams(**base)

    def to_c(self) -> RenderParamsC:
        p = RenderParamsC()
        p.width, p.height = int(self.width), int(self.height)
        p.spp, p.spp_offset, p.spp_chunk = int(self.spp), int(self.spp_offset), int(self.spp_chunk)
        p.max_depth, p.illum, p.fov_deg = int(self.max_depth), float(self.illum), float(self.fov_deg)
        p.eye[:] = [float(x) for x in self.eye]
        p.dir[:] = [float(x) for x in self.direction]
        p.up[:] = [float(x) for x in self.up]
        p.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        p.prev_count = int(self.prev_count)
        p.fresnel_kd = 1 if self.fresnel_kd else 0
        p.tile, p.shard_count, p.shard_index = int(self.tile), int(self.shard_count), int(self.shard_index)
        p.packed = 1 if self.packed else 0
        if self.pipeline not in PIPELINES:
            raise ValueError(f"pipeline must be one of {sorted(PIPELINES)}")
        p.pipeline = PIPELINES[self.pipeline]
        p.wf_batch = int(self.wf_batch)
        if self.mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        p.mode = MODES[self.mode]
        p.lean = 1 if self.lean else 0
        p.wf_sort = 1 if self.wf_sort else 0
        p.wf_streams, p.wf_refill, p.wf_group_shift = int(self.wf_streams), int(self.wf_refill), int(self.wf_group_shift)
        p.ready_thresh, p.tail_units_per_lane = int(self.ready_thresh), int(self.tail_units_per_lane)
        p.tail_units, p.wf_mem_limit = int(self.tail_units), int(self.wf_mem_limit)
        p.force_peer_copy = 1 if self.force_peer_copy else 0
        if self.gather not in GATHERS:
            raise ValueError(f"gather must be one of {sorted(GATHERS)}")
        p.gather = GATHERS[self.gather]
        return p

    def output_pixels(self) -> int:
        if self.packed or self.shard_count > 1:
            return int(lib().mcpt_shard_pixel_count(C.byref(self.to_c())))
        return int(self.width) * int(self.height)

    def shard_pixels(self) -> np.ndarray:
        """(n, 2) int32 (x, y) of every output slot of a packed/sharded render (-1 = padding)."""
        p = self.to_c()
        n = int(check(lib().mcpt_shard_pixel_count(C.byref(p))))
        xy = np.zeros((n, 2), np.int32)
        check(lib().mcpt_shard_pixels(C.byref(p), xy.ctypes.data_as(C.POINTER(C.c_int32))))
        return xy


class Scene:
    """A device-resident scene (CreateGeometry result + KD tree)."""

    LAYOUTS = {"auto": _capi.LAYOUT_AUTO, "global": _capi.LAYOUT_GLOBAL}
    KD_BUILDS = {"reference": _capi.KD_BUILD_REFERENCE, "sah": _capi.KD_BUILD_SAH}

    def __init__(self, model: ObjModel, host_only: bool = False, kd_cache: Optional[str] = None,
                 layout: str = "auto", kd_build: str = "reference"):
        """kd_cache: directory for the on-disk KD-build cache (mcpt_scene_create_ex);
        ``cache_hit`` tells whether the tree was read from it.  layout "global":
        the scene image with child-box pair records in global memory even if it
        would fit in LDS (MCPT_LAYOUT_GLOBAL).  kd_build "sah": the KD tree's
        splits by the SAH with a traversal cost (MCPT_KD_BUILD_SAH) instead of
        QuinEngine's KDTree.hpp rule -- the same image, fewer node visits."""
        if layout not in self.LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(self.LAYOUTS)}")
        if kd_build not in self.KD_BUILDS:
            raise ValueError(f"kd_build must be one of {sorted(self.KD_BUILDS)}")
        h = C.c_void_p()
        if kd_cache:
            os.makedirs(kd_cache, exist_ok=True)
        opt = _capi.SceneOptions(os.fsencode(kd_cache) if kd_cache else None, int(host_only), self.LAYOUTS[layout],
                                 self.KD_BUILDS[kd_build])
        hit = C.c_int32(0)
        check(lib().mcpt_scene_create_ex(model.handle, C.byref(opt), C.byref(h), C.byref(hit)))
        self.cache_hit = bool(hit.value)
        self._h = h
        self.host_only = host_only

    def close(self):
        h = getattr(self, "_h", None)   # None also when __init__ failed
        if h is not None and _capi._lib is not None:
            _capi._lib.mcpt_scene_destroy(h)
        self._h = None

    __del__ = close

    @property
    def handle(self):
        if self._h is None:
            raise McptError(-1, "scene destroyed")
        return self._h

    def info(self) -> dict:
        i = _capi.SceneInfo()
        check(lib().mcpt_scene_get_info(self.handle, C.byref(i)))
        d = {n: int(getattr(i, n)) for n, _ in i._fields_}
        # emitter boxes of the wavefront's terminal cull; 0: the scene does not allow it
        d["terminal_cull_boxes"] = int(lib().mcpt_scene_terminal_cull_boxes(self.handle))
        # occluder boxes of the wavefront's miss cull; 0: the scene has none
        d["miss_cull_boxes"] = int(lib().mcpt_scene_miss_cull_boxes(self.handle, None))
        # the wavefront's direct lists: triangles a small box may hold (0: built without), and the small boxes
        bt = np.zeros(8, np.uint32)
        k = int(lib().mcpt_scene_direct_lists(self.handle, None, bt.ctypes.data_as(C.POINTER(C.c_uint32)), None, None))
        d["direct_list_k"] = k
        d["direct_list_boxes"] = int(((bt >= 1) & (bt <= k)).sum()) if k else 0
        return d

    def miss_cull_boxes(self) -> np.ndarray:
        """(n, 6) float32 occluder boxes of the miss cull: min xyz, max xyz."""
        b = np.zeros((16, 6), np.float32)
        n = int(lib().mcpt_scene_miss_cull_boxes(self.handle, _fptr(b)))
        return b[:n]

    def direct_lists(self) -> dict:
        """The wavefront's direct lists: {"k", "tri_box" (kd id -> occluder box), "box_tris"
        (triangles per box), "lists" ((boxes, k) record indices of the small boxes' triangles,
        image order), "list_kd" (the same as kd ids, -1 past a list's end), "counts" (per box:
        the length of its list, 0 = its rays walk)}; k is 0 for a library built without them."""
        n = int(lib().mcpt_scene_miss_cull_boxes(self.handle, None))
        nt = self.info()["n_triangles"]
        tri_box = np.full(max(nt, 1), -1, np.int32)
        box_tris = np.zeros(8, np.uint32)
        lists = np.zeros(8 * 16, np.uint32)
        list_kd = np.full(8 * 16, -1, np.int32)
        k = int(lib().mcpt_scene_direct_lists(self.handle, tri_box.ctypes.data_as(C.POINTER(C.c_int32)),
                                              box_tris.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              lists.ctypes.data_as(C.POINTER(C.c_uint32)),
                                              list_kd.ctypes.data_as(C.POINTER(C.c_int32))))
        box_tris = box_tris[:n] if k else box_tris[:0]
        counts = np.where(box_tris <= k, box_tris, 0).astype(np.uint32)
        return {"k": k, "tri_box": tri_box[:nt] if k else tri_box[:0], "box_tris": box_tris,
                "lists": lists[: 8 * k].reshape(8, k)[: len(box_tris)] if k else lists[:0].reshape(0, 0),
                "list_kd": list_kd[: 8 * k].reshape(8, k)[: len(box_tris)] if k else list_kd[:0].reshape(0, 0),
                "counts": counts}

    def clip_spheres(self) -> dict:
        """The sphere clip's spheres: {"mask" (bit i: occluder box i has one), "spheres" ((8, 4)
        float32 {centre xyz, radius^2}, zeros for a box without one)}."""
        sp = np.zeros((8, 4), np.float32)
        return {"mask": int(lib().mcpt_scene_clip_spheres(self.handle, _fptr(sp))), "spheres": sp}

    def _render_stats(self, st) -> dict:
        d = st.as_dict()
        for name in (
            # secondary rays resolved from a box's list instead of a walk (lean wavefront renders)
            "direct_rays",
            # rays the wavefront's secondary extends walked (0: megakernel, or built without the direct resolve)
            "extend_rays",
            # of those, the rays an extend started with a box selector (0: built without the clip walk)
            "clipped_rays",
            # paths whose bounce 0 the kernel that resolved their primary rays also shaded (0: every other render)
            "primary_shaded",
            # clipped rays whose walk a box's sphere left nothing of (0: a render that does not clip to spheres)
            "sphere_skips",
        ):
            d[name] = int(getattr(lib(), "mcpt_scene_" + name)(self.handle))
        return d

    def primary_tile_classes(self):
        """The last render's primary lists: owned 8x8 tiles by candidate count --
        {"empty", "listed", "walked", "k"}; all three counts are 0 after a render
        that did not resolve its primary rays from tile lists."""
        out = (C.c_uint32 * 4)()
        check(lib().mcpt_scene_primary_tile_classes(self.handle, out))
        return {"empty": int(out[0]), "listed": int(out[1]), "walked": int(out[2]), "k": int(out[3])}

    def kd(self):
        """(nodes (n,12) u32, leaf ids, kd_tris, geoms (g,14) f32) as built."""
        i = self.info()
        nodes = np.zeros((i["n_nodes"], 12), np.uint32)
        leafs = np.zeros(max(i["n_leaf_refs"], 1), np.uint32)
        kdt = np.zeros(i["n_triangles"], np.int32)
        geoms = np.zeros((i["n_geometries"], 14), np.float32)
        check(lib().mcpt_scene_copy_kd(self.handle, nodes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       leafs.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       kdt.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(geoms)))
        return nodes, leafs[: i["n_leaf_refs"]], kdt, geoms

    def render(self, params: RenderParams, fb: Optional[np.ndarray] = None):
        """Synchronous render into a host float32 RGB buffer; returns (fb, stats)."""
        n = params.output_pixels()
        if fb is None:
            fb = np.zeros((n, 3) if (params.packed or params.shard_count > 1) else (params.height, params.width, 3),
                          np.float32)
        if fb.dtype != np.float32 or not fb.flags.c_contiguous or fb.size != 3 * n:
            raise McptError(-1, "fb must be a C-contiguous float32 array with 3 floats per output pixel")
        st = RenderStats()
        check(lib().mcpt_render(self.handle, C.byref(params.to_c()), _fptr(fb), C.byref(st)))
        return fb, self._render_stats(st)

    def intersect(self, o: np.ndarray, d: np.ndarray, t_max: float = 3.402823466e38):
        """Closest hits of rays (origins o, directions d: (n, 3) float32) on the
        device (CUTracer.cu:44-96 through the render traversal): (kd triangle id
        or -1, (n, 3) beta gamma t, counters)."""
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise McptError(-1, "o and d must have the same shape")
        n = o.shape[0]
        tri = np.zeros(n, np.int32)
        hit = np.zeros((n, 3), np.float32)
        st = RenderStats()
        check(lib().mcpt_intersect(self.handle, n, _fptr(o), _fptr(d), C.c_float(t_max),
                                   tri.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(hit), C.byref(st)))
        return tri, hit, st.as_dict()

    def trace_device(self, n: int, o_ptr: int, d_ptr: int, tri_ptr: int, hit_ptr: int = 0, t_max_ptr: int = 0,
                     stream_ptr: int = 0, **params):
        """Closest hits of n rays in device memory (mcpt_trace_device), asynchronous on the
        stream: o / d (n, 3) float32, tri (n,) int32 = kd triangle id or -1, hit (n, 3) float32
        beta gamma t (optional), t_max (n,) float32 (optional: params' t_max for all).  What
        ``intersect`` returns for the same rays, without leaving the device.  params: the fields
        of ``trace_params``.  Run it on the stream of the scene's renders, or synchronize."""
        check(lib().mcpt_trace_device(self.handle, C.byref(trace_params(**params)), int(n), C.c_void_p(o_ptr),
                                      C.c_void_p(d_ptr), C.c_void_p(t_max_ptr), C.c_void_p(tri_ptr),
                                      C.c_void_p(hit_ptr), C.c_void_p(stream_ptr)))

    def occluded_device(self, n: int, o_ptr: int, d_ptr: int, occluded_ptr: int, t_max_ptr: int = 0,
                        stream_ptr: int = 0, **params):
        """Any-hit query of n rays in device memory (mcpt_occluded_device): occluded (n,) uint8 =
        1 where some triangle is hit with t < t_max -- (tri >= 0) of ``trace_device`` for the same
        rays, from a walk that stops at its first accepted triangle."""
        check(lib().mcpt_occluded_device(self.handle, C.byref(trace_params(**params)), int(n), C.c_void_p(o_ptr),
                                         C.c_void_p(d_ptr), C.c_void_p(t_max_ptr), C.c_void_p(occluded_ptr),
                                         C.c_void_p(stream_ptr)))

    def occluded(self, o: np.ndarray, d: np.ndarray, t_max=None, **params):
        """Any-hit query of host rays (mcpt_occluded), synchronous: (uint8 array, counters of this
        call).  t_max: None, a scalar for all rays, or one value per ray."""
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise McptError(-1, "o and d must have the same shape")
        n = o.shape[0]
        tm = None
        if t_max is not None and np.ndim(t_max) == 0:
            params = {**params, "t_max": float(t_max)}
        elif t_max is not None:
            tm = np.ascontiguousarray(t_max, np.float32).reshape(-1)
            if tm.shape[0] != n:
                raise McptError(-1, "t_max must hold one value per ray")
        occ = np.zeros(n, np.uint8)
        st = RenderStats()
        check(lib().mcpt_occluded(self.handle, C.byref(trace_params(**params)), n, _fptr(o), _fptr(d),
                                  _fptr(tm) if tm is not None else None, occ.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  C.byref(st)))
        return occ, st.as_dict()

    def trace_stats(self) -> dict:
        """Counters of the device ray queries since the last read (mcpt_trace_stats_read): waits
        for them and resets.  The render stats (``stats``) are separate."""
        st = RenderStats()
        check(lib().mcpt_trace_stats_read(self.handle, C.byref(st)))
        return st.as_dict()

    def reserve_rays(self):
        """Allocate what the ray queries need (mcpt_scene_reserve_rays): later queries allocate nothing."""
        check(lib().mcpt_scene_reserve_rays(self.handle))

    def radiance_device(self, n: int, o_ptr: int, d_ptr: int, out_ptr: int, stream_ids_ptr: int = 0,
                        stream_ptr: int = 0, **params):
        """Path-traced radiance along n rays in device memory (mcpt_radiance_device), asynchronous
        on the stream: o / d (n, 3) float32, used as given; out (n, 4) float32 = the mean of spp
        samples (r, g, b, 0), read first when prev_count > 0; stream ids (n,) uint32, optional
        (the ray's index): the id takes the pixel's place in the RNG seed, so a render's primary
        rays with their pixel indices give that render's samples.  CVMCTracer mode.  params: the
        fields of ``radiance_params``.  Counted in ``trace_stats``.  Run it on the stream of the
        scene's renders, or synchronize."""
        check(lib().mcpt_radiance_device(self.handle, C.byref(radiance_params(**params)), int(n), C.c_void_p(o_ptr),
                                         C.c_void_p(d_ptr), C.c_void_p(stream_ids_ptr), C.c_void_p(out_ptr),
                                         C.c_void_p(stream_ptr)))

    def radiance(self, o: np.ndarray, d: np.ndarray, stream_ids=None, prev=None, **params):
        """Radiance along host rays (mcpt_radiance), synchronous: ((n, 3) float32, counters of this
        call).  prev: the earlier mean the running mean continues (with prev_count > 0)."""
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise McptError(-1, "o and d must have the same shape")
        n = o.shape[0]
        ids = None
        if stream_ids is not None:
            ids = np.ascontiguousarray(stream_ids, np.uint32).reshape(-1)
            if ids.shape[0] != n:
                raise McptError(-1, "stream_ids must hold one value per ray")
        out = np.zeros((n, 3), np.float32)
        if prev is not None:
            out[...] = np.asarray(prev, np.float32).reshape(n, 3)
        st = RenderStats()
        check(lib().mcpt_radiance(self.handle, C.byref(radiance_params(**params)), n, _fptr(o), _fptr(d),
                                  ids.ctypes.data_as(C.POINTER(C.c_uint32)) if ids is not None else None,
                                  _fptr(out), C.byref(st)))
        return out, st.as_dict()

    def reserve_radiance(self, n: int, **params):
        """Allocate what a radiance query of n rays with these params needs
        (mcpt_scene_reserve_radiance): a later query that needs no more allocates nothing."""
        check(lib().mcpt_scene_reserve_radiance(self.handle, C.byref(radiance_params(**params)), int(n)))

    def radiance_ex_device(self, n: int, o_ptr: int, d_ptr: int, out_ptr: int, stream_ids_ptr: int = 0,
                           stream_ptr: int = 0, **params):
        """``radiance_device`` with the pipeline as a parameter (mcpt_radiance_ex_device).  params:
        the fields of ``radiance_ex_params`` -- those of ``radiance_params``, ``pipeline``
        ("megakernel", the default: exactly ``radiance_device``; "wavefront": the rays run as a
        wavefront render of n pixels, same bits) and the wavefront's wf_batch, wf_streams,
        wf_refill, wf_group_shift, wf_sort, wf_mem_limit (scheduling only).  Counted in
        ``trace_stats``; on the wavefront a lean query counts rays, paths and shades."""
        check(lib().mcpt_radiance_ex_device(self.handle, C.byref(radiance_ex_params(**params)), int(n),
                                            C.c_void_p(o_ptr), C.c_void_p(d_ptr), C.c_void_p(stream_ids_ptr),
                                            C.c_void_p(out_ptr), C.c_void_p(stream_ptr)))

    def radiance_ex(self, o: np.ndarray, d: np.ndarray, stream_ids=None, prev=None, **params):
        """``radiance`` with the pipeline as a parameter (mcpt_radiance_ex), synchronous: ((n, 3)
        float32, counters of this call; ``variant`` 4 / 5 on the wavefront)."""
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise McptError(-1, "o and d must have the same shape")
        n = o.shape[0]
        ids = None
        if stream_ids is not None:
            ids = np.ascontiguousarray(stream_ids, np.uint32).reshape(-1)
            if ids.shape[0] != n:
                raise McptError(-1, "stream_ids must hold one value per ray")
        out = np.zeros((n, 3), np.float32)
        if prev is not None:
            out[...] = np.asarray(prev, np.float32).reshape(n, 3)
        st = RenderStats()
        check(lib().mcpt_radiance_ex(self.handle, C.byref(radiance_ex_params(**params)), n, _fptr(o), _fptr(d),
                                     ids.ctypes.data_as(C.POINTER(C.c_uint32)) if ids is not None else None,
                                     _fptr(out), C.byref(st)))
        return out, st.as_dict()

    def reserve_radiance_ex(self, n: int, **params):
        """Allocate what a query of n rays with these ``radiance_ex_params`` needs
        (mcpt_scene_reserve_radiance_ex): a later query that needs no more allocates nothing."""
        check(lib().mcpt_scene_reserve_radiance_ex(self.handle, C.byref(radiance_ex_params(**params)), int(n)))

    def query_route_rays(self):
        """(direct, extend, clipped, sphere_skips) rays of the wavefront radiance queries in the
        record ``trace_stats`` last read (mcpt_scene_query_route_rays)."""
        out = (C.c_uint64 * 4)()
        check(lib().mcpt_scene_query_route_rays(self.handle, out))
        return tuple(int(v) for v in out)

    def ao_device(self, n: int, p_ptr: int, n_ptr: int, out_ptr: int, stream_ids_ptr: int = 0,
                  stream_ptr: int = 0, **params):
        """Ambient occlusion of n points in device memory (mcpt_ao_device), asynchronous on the
        stream: p / normals (n, 3) float32, the normals unit length and used as given; out (n,)
        float32 = the share of spp cosine-hemisphere rays of length ``radius`` from p + bias * dir
        that reach nothing (1 = open), read first when prev_count > 0; stream ids (n,) uint32,
        optional (the point's index), as ``radiance_device``.  Counted in integers: scheduling
        never changes a bit.  params: the fields of ``ao_params``.  Counted in ``trace_stats``.
        Run it on the stream of the scene's renders, or synchronize."""
        check(lib().mcpt_ao_device(self.handle, C.byref(ao_params(**params)), int(n), C.c_void_p(p_ptr),
                                   C.c_void_p(n_ptr), C.c_void_p(stream_ids_ptr), C.c_void_p(out_ptr),
                                   C.c_void_p(stream_ptr)))

    def ao(self, p: np.ndarray, normals: np.ndarray, stream_ids=None, prev=None, **params):
        """Ambient occlusion of host points (mcpt_ao), synchronous: ((n,) float32, counters of this
        call).  prev: the earlier mean the running mean continues (with prev_count > 0)."""
        p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if p.shape != normals.shape:
            raise McptError(-1, "p and normals must have the same shape")
        n = p.shape[0]
        ids = None
        if stream_ids is not None:
            ids = np.ascontiguousarray(stream_ids, np.uint32).reshape(-1)
            if ids.shape[0] != n:
                raise McptError(-1, "stream_ids must hold one value per point")
        out = np.zeros(n, np.float32)
        if prev is not None:
            out[...] = np.asarray(prev, np.float32).reshape(n)
        st = RenderStats()
        check(lib().mcpt_ao(self.handle, C.byref(ao_params(**params)), n, _fptr(p), _fptr(normals),
                            ids.ctypes.data_as(C.POINTER(C.c_uint32)) if ids is not None else None, _fptr(out),
                            C.byref(st)))
        return out, st.as_dict()

    def render_ao_device(self, params: RenderParams, out_ptr: int, stream_ptr: int = 0, **ao):
        """Ambient occlusion at the first hits of a frame's own primary rays
        (mcpt_render_ao_device), asynchronous: out (H, W) float32, 1 where a pixel's samples miss
        the scene or see nothing within ``radius`` of their hits.  The frame, its samples, seed
        and prev_count come from ``params``; ao: radius, lean, workgroups, refill, unit_samples."""
        check(lib().mcpt_render_ao_device(self.handle, C.byref(params.to_c()), C.byref(ao_params(**ao)),
                                          C.c_void_p(out_ptr), C.c_void_p(stream_ptr)))

    def render_ao(self, params: RenderParams, prev: Optional[np.ndarray] = None, **ao):
        """``render_ao_device`` into a host array (mcpt_render_ao), synchronous: ((H, W) float32,
        counters of this call).  prev: the earlier mean (with ``params.prev_count > 0``)."""
        out = np.zeros((int(params.height), int(params.width)), np.float32)
        if prev is not None:
            out[...] = np.asarray(prev, np.float32).reshape(out.shape)
        st = RenderStats()
        check(lib().mcpt_render_ao(self.handle, C.byref(params.to_c()), C.byref(ao_params(**ao)), _fptr(out),
                                   C.byref(st)))
        return out, st.as_dict()

    def reserve_ao(self, n: int):
        """Allocate what an ambient-occlusion query of n points, or of a frame of n pixels, needs
        (mcpt_scene_reserve_ao): a later query that needs no more allocates nothing."""
        check(lib().mcpt_scene_reserve_ao(self.handle, int(n)))

    def lights(self):
        """The scene's light table (mcpt_scene_lights): the emitters' triangles the direct-lighting
        queries sample, as a dict -- ``kd_ids`` (L,) int32 ascending, ``cdf`` (L,) float32 ending at
        1.0, ``normals`` (L, 3) float32, ``area_total`` float.  Works on host-only scenes."""
        n = lib().mcpt_scene_lights(self.handle, None, None, None, None)
        ids = np.zeros(n, np.int32)
        cdf = np.zeros(n, np.float32)
        nrm = np.zeros((n, 3), np.float32)
        area = C.c_float(0.0)
        lib().mcpt_scene_lights(self.handle, ids.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(cdf), _fptr(nrm),
                                C.byref(area))
        return {"kd_ids": ids, "cdf": cdf, "normals": nrm, "area_total": np.float32(area.value)}

    def direct_device(self, n: int, p_ptr: int, n_ptr: int, out_ptr: int, stream_ids_ptr: int = 0,
                      stream_ptr: int = 0, **params):
        """Direct lighting of n points in device memory (mcpt_direct_device), asynchronous on the
        stream: p / normals (n, 3) float32, the normals unit length and used as given; out (n, 4)
        float32 = (r, g, b, 0), the cosine-weighted mean of the emitter radiance over the point's
        hemisphere (E / pi) from spp area samples of the scene's lights, read first when
        prev_count > 0; stream ids (n,) uint32, optional (the point's index), as ``ao_device``.
        ``spp_chunk`` is part of the result (the summation order); the scheduling fields never
        change a bit.  params: the fields of ``direct_params``.  Counted in ``trace_stats``.  Run
        it on the stream of the scene's renders, or synchronize."""
        check(lib().mcpt_direct_device(self.handle, C.byref(direct_params(**params)), int(n), C.c_void_p(p_ptr),
                                       C.c_void_p(n_ptr), C.c_void_p(stream_ids_ptr), C.c_void_p(out_ptr),
                                       C.c_void_p(stream_ptr)))

    def direct(self, p: np.ndarray, normals: np.ndarray, stream_ids=None, prev=None, **params):
        """Direct lighting of host points (mcpt_direct), synchronous: ((n, 3) float32, counters of
        this call).  prev: the earlier mean the running mean continues (with prev_count > 0)."""
        p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if p.shape != normals.shape:
            raise McptError(-1, "p and normals must have the same shape")
        n = p.shape[0]
        ids = None
        if stream_ids is not None:
            ids = np.ascontiguousarray(stream_ids, np.uint32).reshape(-1)
            if ids.shape[0] != n:
                raise McptError(-1, "stream_ids must hold one value per point")
        out = np.zeros((n, 3), np.float32)
        if prev is not None:
            out[...] = np.asarray(prev, np.float32).reshape(n, 3)
        st = RenderStats()
        check(lib().mcpt_direct(self.handle, C.byref(direct_params(**params)), n, _fptr(p), _fptr(normals),
                                ids.ctypes.data_as(C.POINTER(C.c_uint32)) if ids is not None else None, _fptr(out),
                                C.byref(st)))
        return out, st.as_dict()

    def render_direct_device(self, params: RenderParams, out_ptr: int, stream_ptr: int = 0, **direct):
        """Direct lighting at the first hits of a frame's own primary rays
        (mcpt_render_direct_device), asynchronous: out (H, W, 4) float32 = (r, g, b, 0), zeros
        where a pixel's samples miss the scene; times ``render_aov``'s albedo it is a diffuse
        surface's direct radiance.  The frame, its samples, seed and prev_count come from
        ``params``; direct: spp_chunk, illum, lean, workgroups, refill."""
        check(lib().mcpt_render_direct_device(self.handle, C.byref(params.to_c()), C.byref(direct_params(**direct)),
                                              C.c_void_p(out_ptr), C.c_void_p(stream_ptr)))

    def render_direct(self, params: RenderParams, prev: Optional[np.ndarray] = None, **direct):
        """``render_direct_device`` into a host array (mcpt_render_direct), synchronous: ((H, W, 3)
        float32, counters of this call).  prev: the earlier mean (with ``params.prev_count > 0``)."""
        out = np.zeros((int(params.height), int(params.width), 3), np.float32)
        if prev is not None:
            out[...] = np.asarray(prev, np.float32).reshape(out.shape)
        st = RenderStats()
        check(lib().mcpt_render_direct(self.handle, C.byref(params.to_c()), C.byref(direct_params(**direct)),
                                       _fptr(out), C.byref(st)))
        return out, st.as_dict()

    def reserve_direct(self, n: int, **params):
        """Allocate what a direct-lighting query of n points, or of a frame of n pixels, with these
        params' spp and spp_chunk needs (mcpt_scene_reserve_direct): a later query that needs no
        more allocates nothing."""
        check(lib().mcpt_scene_reserve_direct(self.handle, C.byref(direct_params(**params)), int(n)))

    def render_unit_counters(self, params: RenderParams):
        """Synchronous render returning (fb, per-unit counters (units, 4): rays, inner, leaf, tests)."""
        n = params.output_pixels()
        fb = np.zeros((n, 3), np.float32)
        chunk = params.spp_chunk if 0 < params.spp_chunk < params.spp else params.spp
        # (a unit per pixel of every owned tile, padding included: more than n on a frame of partial tiles)
        units = int(lib().mcpt_shard_pixel_count(C.byref(params.to_c()))) * ((params.spp + chunk - 1) // chunk)
        uc = np.zeros((units, 4), np.uint32)
        check(lib().mcpt_render_unit_counters(self.handle, C.byref(params.to_c()), _fptr(fb),
                                              uc.ctypes.data_as(C.POINTER(C.c_uint32))))
        return fb, uc

    def render_device(self, params: RenderParams, d_fb_rgba_ptr: int, stream_ptr: int = 0):
        """Asynchronous render into a device RGBA float buffer (e.g. a torch tensor's data_ptr())."""
        check(lib().mcpt_render_device(self.handle, C.byref(params.to_c()), C.c_void_p(d_fb_rgba_ptr),
                                       C.c_void_p(stream_ptr)))

    def render_aov(self, params: RenderParams, albedo_cov: Optional[np.ndarray] = None,
                   normal_depth: Optional[np.ndarray] = None):
        """First-hit feature buffers of the render's own primary rays (mcpt_render_aov):
        (albedo_cov, normal_depth), float32 (H, W, 4) each -- r g b coverage and
        nx ny nz t, means over ``params.spp`` samples (a few are plenty).  With
        ``prev_count > 0`` the given buffers are blended in by the linear running mean."""
        shape = (int(params.height), int(params.width), 4)
        bufs = []
        for a in (albedo_cov, normal_depth):
            if a is None:
                a = np.zeros(shape, np.float32)
            if a.dtype != np.float32 or not a.flags.c_contiguous or a.size != shape[0] * shape[1] * 4:
                raise McptError(-1, "feature buffers must be C-contiguous float32 arrays with 4 floats per pixel")
            bufs.append(a)
        check(lib().mcpt_render_aov(self.handle, C.byref(params.to_c()), _fptr(bufs[0]), _fptr(bufs[1])))
        return bufs[0], bufs[1]

    def render_aov_device(self, params: RenderParams, albedo_ptr: int, nd_ptr: int, stream_ptr: int = 0):
        """Asynchronous feature buffers into two device RGBA float buffers (mcpt_render_aov_device)."""
        check(lib().mcpt_render_aov_device(self.handle, C.byref(params.to_c()), C.c_void_p(albedo_ptr),
                                           C.c_void_p(nd_ptr), C.c_void_p(stream_ptr)))

    def render_var(self, params: RenderParams, fb: Optional[np.ndarray] = None, var: Optional[np.ndarray] = None):
        """``render`` plus the per-pixel variance of this call's pixel mean (mcpt_render_var):
        (fb (H, W, 3), var (H, W, 4) = var_r var_g var_b 0, stats).  A batch-means estimate
        over the render's chunks, so ``spp_chunk`` must cut ``spp`` into at least two; linear
        radiance squared in both modes.  With ``prev_count > 0`` the given buffers are blended in."""
        H, W = int(params.height), int(params.width)
        if fb is None:
            fb = np.zeros((H, W, 3), np.float32)
        if var is None:
            var = np.zeros((H, W, 4), np.float32)
        if fb.dtype != np.float32 or not fb.flags.c_contiguous or fb.size != 3 * H * W:
            raise McptError(-1, "fb must be a C-contiguous float32 array with 3 floats per pixel")
        if var.dtype != np.float32 or not var.flags.c_contiguous or var.size != 4 * H * W:
            raise McptError(-1, "var must be a C-contiguous float32 array with 4 floats per pixel")
        st = RenderStats()
        check(lib().mcpt_render_var(self.handle, C.byref(params.to_c()), _fptr(fb), _fptr(var), C.byref(st)))
        return fb, var, self._render_stats(st)

    def render_var_device(self, params: RenderParams, d_fb_rgba_ptr: int, d_var_rgba_ptr: int, stream_ptr: int = 0):
        """Asynchronous render and variance into two device RGBA float buffers (mcpt_render_var_device)."""
        check(lib().mcpt_render_var_device(self.handle, C.byref(params.to_c()), C.c_void_p(d_fb_rgba_ptr),
                                           C.c_void_p(d_var_rgba_ptr), C.c_void_p(stream_ptr)))

    def render_adaptive(self, params: RenderParams, adaptive=None, fb: Optional[np.ndarray] = None,
                        var: Optional[np.ndarray] = None):
        """Variance-driven adaptive sampling (mcpt_render_adaptive): passes of ``params.spp`` samples,
        each only over the pixels whose luminance standard error is still above the threshold
        (``adaptive``: an ``adaptive_params(...)``, None = the defaults).  Returns (fb (H, W, 3),
        var (H, W, 4), count (H, W) uint32 = passes each pixel received, stats summed over the
        passes).  A pixel with count m holds what m chained uniform ``render_var`` calls leave in it."""
        H, W = int(params.height), int(params.width)
        if fb is None:
            fb = np.zeros((H, W, 3), np.float32)
        if var is None:
            var = np.zeros((H, W, 4), np.float32)
        if fb.dtype != np.float32 or not fb.flags.c_contiguous or fb.size != 3 * H * W:
            raise McptError(-1, "fb must be a C-contiguous float32 array with 3 floats per pixel")
        if var.dtype != np.float32 or not var.flags.c_contiguous or var.size != 4 * H * W:
            raise McptError(-1, "var must be a C-contiguous float32 array with 4 floats per pixel")
        count = np.zeros((max(H, 0), max(W, 0)), np.uint32)
        st = RenderStats()
        check(lib().mcpt_render_adaptive(self.handle, C.byref(params.to_c()),
                                         C.byref(adaptive) if adaptive is not None else None, _fptr(fb), _fptr(var),
                                         count.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st)))
        return fb, var, count, self._render_stats(st)

    def render_adaptive_device(self, params: RenderParams, adaptive, d_fb_rgba_ptr: int, d_var_rgba_ptr: int,
                               d_count_ptr: int, stream_ptr: int = 0):
        """Adaptive render into device buffers (mcpt_render_adaptive_device): RGBA float framebuffer
        and variance, one uint32 per pixel of pass counts.  Waits for the stream once per listed pass."""
        check(lib().mcpt_render_adaptive_device(self.handle, C.byref(params.to_c()),
                                                C.byref(adaptive) if adaptive is not None else None,
                                                C.c_void_p(d_fb_rgba_ptr), C.c_void_p(d_var_rgba_ptr),
                                                C.c_void_p(d_count_ptr), C.c_void_p(stream_ptr)))

    def render_adaptive_ex(self, params: RenderParams, adaptive=None, fb: Optional[np.ndarray] = None,
                           var: Optional[np.ndarray] = None):
        """``render_adaptive`` with ``params.pipeline`` honoured (mcpt_render_adaptive_ex): on the
        wavefront a listed pass is a wavefront render of the listed pixels.  Same arguments, same
        returns, the same fb, var and count bit for bit; ``render_adaptive`` is the megakernel-only
        form."""
        H, W = int(params.height), int(params.width)
        if fb is None:
            fb = np.zeros((H, W, 3), np.float32)
        if var is None:
            var = np.zeros((H, W, 4), np.float32)
        if fb.dtype != np.float32 or not fb.flags.c_contiguous or fb.size != 3 * H * W:
            raise McptError(-1, "fb must be a C-contiguous float32 array with 3 floats per pixel")
        if var.dtype != np.float32 or not var.flags.c_contiguous or var.size != 4 * H * W:
            raise McptError(-1, "var must be a C-contiguous float32 array with 4 floats per pixel")
        count = np.zeros((max(H, 0), max(W, 0)), np.uint32)
        st = RenderStats()
        check(lib().mcpt_render_adaptive_ex(self.handle, C.byref(params.to_c()),
                                            C.byref(adaptive) if adaptive is not None else None, _fptr(fb),
                                            _fptr(var), count.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st)))
        return fb, var, count, self._render_stats(st)

    def render_adaptive_ex_device(self, params: RenderParams, adaptive, d_fb_rgba_ptr: int, d_var_rgba_ptr: int,
                                  d_count_ptr: int, stream_ptr: int = 0):
        """``render_adaptive_device`` with ``params.pipeline`` honoured (mcpt_render_adaptive_ex_device)."""
        check(lib().mcpt_render_adaptive_ex_device(self.handle, C.byref(params.to_c()),
                                                   C.byref(adaptive) if adaptive is not None else None,
                                                   C.c_void_p(d_fb_rgba_ptr), C.c_void_p(d_var_rgba_ptr),
                                                   C.c_void_p(d_count_ptr), C.c_void_p(stream_ptr)))

    def reserve(self, params: RenderParams):
        check(lib().mcpt_scene_reserve(self.handle, C.byref(params.to_c())))

    def plan(self, params: RenderParams) -> dict:
        """The scheduling a render of `params` would use (streams, batch, thresholds) and
        its device memory (mcpt_plan_query); nothing is allocated or launched."""
        out = _capi.PlanInfo()
        check(lib().mcpt_plan_query(self.handle, C.byref(params.to_c()), C.byref(out)))
        return out.as_dict()

    def stats(self) -> dict:
        st = RenderStats()
        check(lib().mcpt_render_stats_read(self.handle, C.byref(st)))
        return self._render_stats(st)


def denoise_params(width: int, height: int, iterations: int = 0, normal_power_log2: int = 0, sigma_z: float = 0.0,
                   albedo_floor: float = 0.0, gamma_space: bool = False) -> "_capi.DenoiseParamsC":
    """mcpt_denoise_params; 0 = the default (5 iterations, normal power 2^7, sigma_z 0.1, floor 0.01)."""
    return _capi.DenoiseParamsC(int(width), int(height), int(iterations), int(normal_power_log2), float(sigma_z),
                                float(albedo_floor), 1 if gamma_space else 0)


def denoise(color: np.ndarray, albedo_cov: np.ndarray, normal_depth: np.ndarray, **params) -> np.ndarray:
    """Edge-avoiding a-trous denoise of a host image on the current device (mcpt_denoise):
    color (H, W, 3) float32, the two feature buffers (H, W, 4) of Scene.render_aov;
    returns the filtered (H, W, 3) image.  params: the fields of denoise_params."""
    color = np.ascontiguousarray(color, np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise McptError(-1, "color must be (H, W, 3)")
    H, W = color.shape[:2]
    a = np.ascontiguousarray(albedo_cov, np.float32)
    n = np.ascontiguousarray(normal_depth, np.float32)
    if a.size != H * W * 4 or n.size != H * W * 4:
        raise McptError(-1, "feature buffers must hold 4 floats per pixel of color")
    out = np.zeros((H, W, 3), np.float32)
    check(lib().mcpt_denoise(C.byref(denoise_params(W, H, **params)), _fptr(color), _fptr(a), _fptr(n), _fptr(out)))
    return out


def denoise_device(width: int, height: int, color_ptr: int, albedo_ptr: int, nd_ptr: int, out_ptr: int,
                   scratch_ptr: int, stream_ptr: int = 0, **params) -> None:
    """Asynchronous denoise of device RGBA float buffers (mcpt_denoise_device): color is only
    read, out receives the result, scratch is a work buffer of the same size."""
    check(lib().mcpt_denoise_device(C.byref(denoise_params(width, height, **params)), C.c_void_p(color_ptr),
                                    C.c_void_p(albedo_ptr), C.c_void_p(nd_ptr), C.c_void_p(out_ptr),
                                    C.c_void_p(scratch_ptr), C.c_void_p(stream_ptr)))


def adaptive_params(max_passes: int = 0, min_passes: int = 0, threshold: float = 0.0, lum_floor: float = 0.0,
                    dilate: int = 0, force_list: bool = False) -> "_capi.AdaptiveParamsC":
    """mcpt_adaptive_params; 0 = the default (8 passes, 1 before selection, threshold 0.2, floor 0.01,
    window radius 1; dilate < 0 = no window)."""
    return _capi.AdaptiveParamsC(int(max_passes), int(min_passes), float(threshold), float(lum_floor), int(dilate),
                                 int(force_list))


TRACE_KINDS = {"closest": _capi.TRACE_CLOSEST, "any": _capi.TRACE_ANY}


def radiance_params(**kw) -> "_capi.RadianceParamsC":
    """mcpt_radiance_params: the library's defaults (spp 1, max_depth 7, illum 10, fresnel_kd 1,
    the renders' seed), then the fields given by name."""
    p = _capi.RadianceParamsC()
    lib().mcpt_radiance_params_default(C.byref(p))
    names = {n for n, _ in _capi.RadianceParamsC._fields_}
    for k, v in kw.items():
        if k not in names:
            raise McptError(-1, f"unknown radiance parameter {k!r}")
        setattr(p, k, float(v) if k == "illum" else int(v))
    return p


def radiance_ex_params(**kw) -> "_capi.RadianceExParamsC":
    """mcpt_radiance_ex_params: the library's defaults (``radiance_params``' in ``base``, the
    megakernel, every wavefront field automatic), then the fields of either struct given by name;
    pipeline: "megakernel" / "wavefront" or the constant."""
    p = _capi.RadianceExParamsC()
    lib().mcpt_radiance_ex_params_default(C.byref(p))
    base = {n for n, _ in _capi.RadianceParamsC._fields_}
    own = {n for n, _ in _capi.RadianceExParamsC._fields_} - {"base"}
    for k, v in kw.items():
        if k in base:
            setattr(p.base, k, float(v) if k == "illum" else int(v))
        elif k == "pipeline":
            p.pipeline = PIPELINES[v] if isinstance(v, str) else int(v)
        elif k in own:
            setattr(p, k, int(v))
        else:
            raise McptError(-1, f"unknown radiance parameter {k!r}")
    return p


def ao_params(**kw) -> "_capi.AoParamsC":
    """mcpt_ao_params: the library's defaults (spp 1, the renders' seed, radius 0 = unbounded,
    bias 0 = 0.01, everything else 0 = automatic), then the fields given by name."""
    p = _capi.AoParamsC()
    lib().mcpt_ao_params_default(C.byref(p))
    names = {n for n, _ in _capi.AoParamsC._fields_}
    for k, v in kw.items():
        if k not in names:
            raise McptError(-1, f"unknown ambient-occlusion parameter {k!r}")
        setattr(p, k, float(v) if k in ("radius", "bias") else int(v))
    return p


def direct_params(**kw) -> "_capi.DirectParamsC":
    """mcpt_direct_params: the library's defaults (spp 1, illum 10, the renders' seed, spp_chunk 0 =
    one chunk, bias 0 = 0.01, everything else 0 = automatic), then the fields given by name."""
    p = _capi.DirectParamsC()
    lib().mcpt_direct_params_default(C.byref(p))
    names = {n for n, _ in _capi.DirectParamsC._fields_}
    for k, v in kw.items():
        if k not in names:
            raise McptError(-1, f"unknown direct-lighting parameter {k!r}")
        setattr(p, k, float(v) if k in ("illum", "bias") else int(v))
    return p


def trace_params(kind="closest", t_max: float = 0.0, lean: bool = False, workgroups: int = 0,
                 refill: int = 0) -> "_capi.TraceParamsC":
    """mcpt_trace_params; t_max 0 = FLT_MAX, workgroups / refill 0 = automatic (scheduling only)."""
    k = TRACE_KINDS[kind] if isinstance(kind, str) else int(kind)
    return _capi.TraceParamsC(k, float(t_max), int(lean), int(workgroups), int(refill))


def denoise_var_params(width: int, height: int, sigma_l: float = 0.0, **params) -> "_capi.DenoiseVarParamsC":
    """mcpt_denoise_var_params: the fields of denoise_params and sigma_l (0 = the default, 4)."""
    return _capi.DenoiseVarParamsC(denoise_params(width, height, **params), float(sigma_l))


def denoise_var(color: np.ndarray, variance: np.ndarray, albedo_cov: np.ndarray, normal_depth: np.ndarray,
                **params) -> np.ndarray:
    """Variance-guided a-trous denoise of a host image on the current device (mcpt_denoise_var):
    color (H, W, 3) float32, variance (H, W, 4) of Scene.render_var, the two feature buffers
    (H, W, 4) of Scene.render_aov; returns the filtered (H, W, 3) image.  params: the fields of
    denoise_var_params."""
    color = np.ascontiguousarray(color, np.float32)
    if color.ndim != 3 or color.shape[2] != 3:
        raise McptError(-1, "color must be (H, W, 3)")
    H, W = color.shape[:2]
    v = np.ascontiguousarray(variance, np.float32)
    a = np.ascontiguousarray(albedo_cov, np.float32)
    n = np.ascontiguousarray(normal_depth, np.float32)
    if v.size != H * W * 4 or a.size != H * W * 4 or n.size != H * W * 4:
        raise McptError(-1, "the variance and feature buffers must hold 4 floats per pixel of color")
    out = np.zeros((H, W, 3), np.float32)
    check(lib().mcpt_denoise_var(C.byref(denoise_var_params(W, H, **params)), _fptr(color), _fptr(v), _fptr(a),
                                 _fptr(n), _fptr(out)))
    return out


def denoise_var_device(width: int, height: int, color_ptr: int, var_ptr: int, albedo_ptr: int, nd_ptr: int,
                       out_ptr: int, scratch_ptr: int, stream_ptr: int = 0, **params) -> None:
    """Asynchronous variance-guided denoise of device RGBA float buffers (mcpt_denoise_var_device):
    color and variance are only read, out receives the result, scratch is a work buffer of the same size."""
    check(lib().mcpt_denoise_var_device(C.byref(denoise_var_params(width, height, **params)), C.c_void_p(color_ptr),
                                        C.c_void_p(var_ptr), C.c_void_p(albedo_ptr), C.c_void_p(nd_ptr),
                                        C.c_void_p(out_ptr), C.c_void_p(scratch_ptr), C.c_void_p(stream_ptr)))


def temporal_params(max_history: int = 0, normal_threshold: float = 0.0, sigma_z: float = 0.0,
                    gamma_space: bool = False) -> "_capi.TemporalParamsC":
    """mcpt_temporal_params; 0 = the default (history capped at 32 frames, normal threshold 0.9,
    sigma_z 0.1)."""
    return _capi.TemporalParamsC(int(max_history), float(normal_threshold), float(sigma_z), 1 if gamma_space else 0)


def temporal(cur: RenderParams, prev: RenderParams, color: np.ndarray, variance, albedo_cov: np.ndarray,
             normal_depth: np.ndarray, hist_color_n: np.ndarray, hist_var, hist_albedo_cov: np.ndarray,
             hist_normal_depth: np.ndarray, **params):
    """Temporal accumulation of host images on the current device (mcpt_temporal): the history
    (hist_color_n (H, W, 4) r g b N, hist_var, the previous frame's feature buffers, camera
    ``prev``) reprojected onto camera ``cur`` and blended with this frame (color (H, W, 3) or
    (H, W, 4), variance of Scene.render_var, the feature buffers of Scene.render_aov).
    variance and hist_var are given together or both None.  Returns (color_n, var), each
    (H, W, 4) -- var None without variance; they and this frame's features are the next
    call's history.  params: the fields of temporal_params."""
    color = np.ascontiguousarray(color, np.float32)
    if color.ndim != 3 or color.shape[2] not in (3, 4):
        raise McptError(-1, "color must be (H, W, 3) or (H, W, 4)")
    H, W = color.shape[:2]
    if color.shape[2] == 3:
        color = np.ascontiguousarray(np.concatenate([color, np.zeros((H, W, 1), np.float32)], axis=-1))
    if (variance is None) != (hist_var is None):
        raise McptError(-1, "variance and hist_var must be given together or both be None")
    bufs = [None if a is None else np.ascontiguousarray(a, np.float32)
            for a in (variance, albedo_cov, normal_depth, hist_color_n, hist_var, hist_albedo_cov, hist_normal_depth)]
    if any(a is not None and a.size != H * W * 4 for a in bufs):
        raise McptError(-1, "every buffer must hold 4 floats per pixel of color")
    v, a, n, hc, hv, ha, hn = bufs
    out = np.zeros((H, W, 4), np.float32)
    out_var = None if v is None else np.zeros((H, W, 4), np.float32)
    opt = lambda x: None if x is None else _fptr(x)   # noqa: E731
    check(lib().mcpt_temporal(C.byref(temporal_params(**params)), C.byref(cur.to_c()), C.byref(prev.to_c()),
                              _fptr(color), opt(v), _fptr(a), _fptr(n), _fptr(hc), opt(hv), _fptr(ha), _fptr(hn),
                              _fptr(out), opt(out_var)))
    return out, out_var


def temporal_device(cur: RenderParams, prev: RenderParams, color_ptr: int, var_ptr: int, albedo_ptr: int, nd_ptr: int,
                    hist_color_ptr: int, hist_var_ptr: int, hist_albedo_ptr: int, hist_nd_ptr: int, out_color_ptr: int,
                    out_var_ptr: int, stream_ptr: int = 0, **params) -> None:
    """Asynchronous temporal accumulation of device RGBA float buffers (mcpt_temporal_device):
    the eight inputs are only read, out_color and out_var receive the result; the three variance
    pointers are given together or all 0 (no variance carried)."""
    check(lib().mcpt_temporal_device(C.byref(temporal_params(**params)), C.byref(cur.to_c()), C.byref(prev.to_c()),
                                     *[C.c_void_p(int(p) or None) for p in
                                       (color_ptr, var_ptr, albedo_ptr, nd_ptr, hist_color_ptr, hist_var_ptr,
                                        hist_albedo_ptr, hist_nd_ptr, out_color_ptr, out_var_ptr)],
                                     C.c_void_p(stream_ptr)))


class Tracer:
    """PW::Tracer as an object: Initialize / CreateGeometry / DestroyGeometry / RenderScene."""

    def __init__(self):
        self.scene: Optional[Scene] = None
        self.last_stats: dict = {}

    def initialize(self, devices: Sequence[int] = (0,)) -> int:   # CUTracer.cu:220-223 (cudaSetDevice(0))
        """devices[0] holds the scene; more entries replicate scenes created afterwards
        on this thread and split each render into interleaved tiles across them,
        gathered to devices[0] (mcpt_init, include/mcpt.h) -- the same image."""
        arr = (C.c_int32 * len(devices))(*devices)
        return check(lib().mcpt_init(arr, len(devices)))

    def create_geometry(self, model: ObjModel) -> int:             # CUTracer.cu:225-314
        self.destroy_geometry()
        self.scene = Scene(model)
        return 0

    def destroy_geometry(self) -> int:                              # CUTracer.cu:316-338
        if self.scene is not None:
            self.scene.close()
            self.scene = None
        return 0

    def render_scene(self, scene_id: int, hostcolor: np.ndarray, num_kernels: int = NUM_KERNELS,
                     samples_per_kernel: int = NUM_SAMPLES_PER_KERNEL, callback=None, **kw) -> int:
        """RenderScene (CUTracer.cu:340-404): num_kernels launches of samples_per_kernel
        samples; after launch k the buffer holds the running mean (prevCount = k).
        Each launch sums its samples of a pixel in sample order, then divides
        (CUTracer.cu:192-214): spp_chunk 0 unless the caller passes another."""
        if self.scene is None:
            raise McptError(-1, "CreateGeometry has not been called")
        H, W = hostcolor.shape[:2]
        stats = {}
        for each in range(num_kernels):
            kw.setdefault("spp_chunk", 0)
            p = RenderParams.for_scene(scene_id, width=W, height=H, spp=samples_per_kernel,
                                       spp_offset=each * samples_per_kernel, prev_count=each, **kw)
            _, st = self.scene.render(p, hostcolor)
            for k, v in st.items():
                stats[k] = stats.get(k, 0) + v if k != "variant" else v
            if callback is not None:
                callback(each, hostcolor)
        self.last_stats = stats
        return 0

    # reference spellings
    Initialize = initialize
    CreateGeometry = create_geometry
    DestroyGeometry = destroy_geometry
    RenderScene = render_scene


_default = Tracer()


def Initialize() -> int:
    return _default.initialize()


def CreateGeometry(model: ObjModel) -> int:
    return _default.create_geometry(model)


def DestroyGeometry() -> int:
    return _default.destroy_geometry()


def RenderScene(sceneID: int, hostcolor: np.ndarray, **kw) -> int:
    return _default.render_scene(sceneID, hostcolor, **kw)


from .imageio import encode_8bit  # noqa: E402,F401  (main.cpp:19-29 encode; kept here for the API)

// capi.cpp -- what the C ABI declared in include/mcpt.h keeps per thread and
// per call rather than per scene: the last error, device selection (the
// reference's Initialize(), CVMCTracer/CUDA/CUTracer.cu:220-223), the parameter
// defaults, the two denoisers and the temporal accumulation in front of them.
// Unlike the reference, no module globals hold
// a scene: every call takes the opaque handle it works on (capi_internal.hpp
// lists the units that implement the rest).
#include <algorithm>
#include <cmath>

#include "aov_launch.hpp"
#include "capi_internal.hpp"
#include "temporal_launch.hpp"
#include "variance_launch.hpp"

namespace mcpt::host {

thread_local std::vector<int> g_devices;
thread_local bool g_peer_ok = true;

namespace {
thread_local std::string g_err;
}

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

}  // namespace mcpt::host

using namespace mcpt::host;

namespace {

// mcpt_denoise_params with its zeros replaced by the defaults; throws on a bad field
mcpt::DenoiseParams denoise_resolve(const mcpt_denoise_params* p) {
    if (!p) throw mcpt::Error{MCPT_E_INVALID, "params is NULL"};
    if (p->width <= 0 || p->height <= 0) throw mcpt::Error{MCPT_E_INVALID, "width/height must be positive"};
    if (p->iterations < 0 || p->iterations > 8) throw mcpt::Error{MCPT_E_INVALID, "iterations must be 0 (default 5) or 1..8"};
    if (p->normal_power_log2 < 0 || p->normal_power_log2 > 10)
        throw mcpt::Error{MCPT_E_INVALID, "normal_power_log2 must be 0 (default 7) or 1..10"};
    if (!(p->sigma_z >= 0.0f) || !std::isfinite(p->sigma_z) || !(p->albedo_floor >= 0.0f) || !std::isfinite(p->albedo_floor))
        throw mcpt::Error{MCPT_E_INVALID, "sigma_z / albedo_floor must be finite and >= 0 (0 = default)"};
    if (p->gamma_space != 0 && p->gamma_space != 1) throw mcpt::Error{MCPT_E_INVALID, "gamma_space must be 0 or 1"};
    mcpt::DenoiseParams d;
    d.width = p->width; d.height = p->height;
    d.iterations = p->iterations ? p->iterations : 5;
    d.normal_power_log2 = p->normal_power_log2 ? p->normal_power_log2 : 7;
    d.sigma_z = p->sigma_z != 0.0f ? p->sigma_z : 0.1f;
    d.albedo_floor = p->albedo_floor != 0.0f ? p->albedo_floor : 0.01f;
    d.gamma_space = p->gamma_space;
    return d;
}

// mcpt_denoise_var_params resolved as denoise_resolve does; sigma_l 0 = 4
mcpt::DenoiseVarParams denoise_var_resolve(const mcpt_denoise_var_params* p) {
    if (!p) throw mcpt::Error{MCPT_E_INVALID, "params is NULL"};
    mcpt::DenoiseVarParams d;
    d.base = denoise_resolve(&p->base);
    if (!(p->sigma_l >= 0.0f) || !std::isfinite(p->sigma_l))
        throw mcpt::Error{MCPT_E_INVALID, "sigma_l must be finite and >= 0 (0 = default)"};
    d.sigma_l = p->sigma_l != 0.0f ? p->sigma_l : 4.0f;
    return d;
}

// Both denoisers on device buffers (arguments non-NULL, params resolved):
// var NULL = the edge-avoiding one (d.sigma_l unused), else the variance-guided
int denoise_on_device(const mcpt::DenoiseVarParams& d, const float* color, const float* var, const float* albedo_cov,
                      const float* normal_depth, float* out, float* scratch, hipStream_t st) {
    const size_t bytes = size_t(d.base.width) * size_t(d.base.height) * 16;
    std::vector<const void*> bufs{color, albedo_cov, normal_depth, out, scratch};
    if (var) bufs.insert(bufs.begin() + 1, var);
    const size_t n = bufs.size() - 2;   // inputs; out and scratch behind them
    for (size_t i = 0; i < bufs.size(); ++i)
        for (size_t j = std::max(i + 1, n); j < bufs.size(); ++j)   // out and scratch against every other buffer
            if (ranges_overlap(bufs[i], bytes, bufs[j], bytes))
                return fail(MCPT_E_INVALID, "the out / scratch buffer overlaps another buffer of the call");
    auto f4 = [](const float* p) { return reinterpret_cast<const float4*>(p); };
    if (var)
        HIP_TRY(mcpt::launch_denoise_var(d, f4(color), f4(var), f4(albedo_cov), f4(normal_depth),
                                         reinterpret_cast<float4*>(out), reinterpret_cast<float4*>(scratch), st));
    else
        HIP_TRY(mcpt::launch_denoise(d.base, f4(color), f4(albedo_cov), f4(normal_depth), reinterpret_cast<float4*>(out),
                                     reinterpret_cast<float4*>(scratch), st));
    return MCPT_OK;
}

// Both denoisers on host arrays, likewise: staged in one temporary allocation
int denoise_on_host(const mcpt::DenoiseVarParams& d, const float* color_rgb, const float* var_rgba,
                    const float* albedo_cov, const float* normal_depth, float* out_rgb) {
    const size_t npx = size_t(d.base.width) * size_t(d.base.height), bytes = npx * 16;
    if (ranges_overlap(out_rgb, npx * 12, color_rgb, npx * 12) ||
        (var_rgba && ranges_overlap(out_rgb, npx * 12, var_rgba, bytes)) ||
        ranges_overlap(out_rgb, npx * 12, albedo_cov, bytes) || ranges_overlap(out_rgb, npx * 12, normal_depth, bytes))
        return fail(MCPT_E_INVALID, "out_rgb overlaps an input");
    // one allocation: colour, variance (if any), albedo_cov, normal_depth, out, scratch
    const auto c = carve({bytes, var_rgba ? bytes : size_t(0), bytes, bytes, bytes, bytes});
    TempDev buf(c.total);
    std::vector<float> rgba(npx * 4, 0.0f);
    rgb_to_rgba(color_rgb, npx, rgba.data());
    HIP_TRY(hipMemcpy(c.at<float>(buf.p, 0), rgba.data(), bytes, hipMemcpyHostToDevice));
    if (var_rgba) HIP_TRY(hipMemcpy(c.at<float>(buf.p, 1), var_rgba, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c.at<float>(buf.p, 2), albedo_cov, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c.at<float>(buf.p, 3), normal_depth, bytes, hipMemcpyHostToDevice));
    const int rc = denoise_on_device(d, c.at<float>(buf.p, 0), var_rgba ? c.at<float>(buf.p, 1) : nullptr,
                                     c.at<float>(buf.p, 2), c.at<float>(buf.p, 3), c.at<float>(buf.p, 4),
                                     c.at<float>(buf.p, 5), nullptr);
    if (rc != MCPT_OK) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(rgba.data(), c.at<float>(buf.p, 4), bytes, hipMemcpyDeviceToHost));
    rgba_to_rgb(rgba.data(), npx, out_rgb);
    return MCPT_OK;
}

// The buffers of a temporal accumulation, device or host: 4 floats per pixel each
struct TemporalBufs {
    const float *color, *var, *albedo_cov, *normal_depth;
    const float *hist_color_n, *hist_var, *hist_albedo_cov, *hist_normal_depth;
    float *out_color_n, *out_var;
};

// Every check of mcpt_temporal / mcpt_temporal_device in the header's order (nothing
// is launched, staged or allocated before it returns); then the kernel's parameters,
// mcpt_temporal_params' zeros replaced by the defaults.  Throws on a failed check
mcpt::TemporalParams temporal_resolve(const mcpt_temporal_params* tp, const mcpt_render_params* cur,
                                      const mcpt_render_params* prev, const TemporalBufs& b) {
    using mcpt::Error;
    if (!cur || !prev || !b.color || !b.albedo_cov || !b.normal_depth || !b.hist_color_n || !b.hist_albedo_cov ||
        !b.hist_normal_depth || !b.out_color_n)
        throw Error{MCPT_E_INVALID, "NULL argument"};
    mcpt_temporal_params t;
    mcpt_temporal_params_default(&t);
    if (tp) {
        if (tp->max_history < 0 || tp->max_history > 65536)
            throw Error{MCPT_E_INVALID, "max_history must be 0 (default 32) or 1..65536"};
        if (!(tp->normal_threshold >= 0.0f && tp->normal_threshold <= 1.0f))
            throw Error{MCPT_E_INVALID, "normal_threshold must be 0 (default 0.9) or in (0, 1]"};
        if (!(tp->sigma_z >= 0.0f) || !std::isfinite(tp->sigma_z))
            throw Error{MCPT_E_INVALID, "sigma_z must be finite and >= 0 (0 = default 0.1)"};
        if (tp->gamma_space != 0 && tp->gamma_space != 1) throw Error{MCPT_E_INVALID, "gamma_space must be 0 or 1"};
        if (tp->max_history) t.max_history = tp->max_history;
        if (tp->normal_threshold != 0.0f) t.normal_threshold = tp->normal_threshold;
        if (tp->sigma_z != 0.0f) t.sigma_z = tp->sigma_z;
        t.gamma_space = tp->gamma_space;
    }
    if (cur->width <= 0 || cur->height <= 0) throw Error{MCPT_E_INVALID, "width/height must be positive"};
    if (cur->mode != MCPT_MODE_CVMCTRACER && cur->mode != MCPT_MODE_QUINENGINE)
        throw Error{MCPT_E_INVALID, "unknown mode"};
    if (prev->width != cur->width) throw Error{MCPT_E_INVALID, "cur and prev differ in width"};
    if (prev->height != cur->height) throw Error{MCPT_E_INVALID, "cur and prev differ in height"};
    if (prev->mode != cur->mode) throw Error{MCPT_E_INVALID, "cur and prev differ in mode"};
    const int nvar = (b.var != nullptr) + (b.hist_var != nullptr) + (b.out_var != nullptr);
    if (nvar != 0 && nvar != 3)
        throw Error{MCPT_E_INVALID, "var, hist_var and out_var must be given together or all be NULL"};
    const uint64_t npx = uint64_t(cur->width) * uint64_t(cur->height);
    if (npx >= (uint64_t(1) << 31) / 3) throw Error{MCPT_E_UNSUPPORTED, "width x height must be below 2^31 / 3"};
    const size_t bytes = size_t(npx) * 16;
    const void* ins[] = {b.color, b.var, b.albedo_cov, b.normal_depth, b.hist_color_n, b.hist_var, b.hist_albedo_cov,
                         b.hist_normal_depth};
    for (const void* out : {static_cast<const void*>(b.out_color_n), static_cast<const void*>(b.out_var)}) {
        if (!out) continue;
        for (const void* in : ins)
            if (in && ranges_overlap(out, bytes, in, bytes))
                throw Error{MCPT_E_INVALID, "an output overlaps an input"};
    }
    if (b.out_var && ranges_overlap(b.out_color_n, bytes, b.out_var, bytes))
        throw Error{MCPT_E_INVALID, "the two outputs overlap"};

    mcpt::TemporalParams k{};
    k.width = cur->width; k.height = cur->height;
    k.mode = cur->mode;
    k.gamma_space = t.gamma_space;
    k.max_n = static_cast<float>(t.max_history - 1);
    k.normal_threshold = t.normal_threshold;
    k.sigma_z = t.sigma_z;
    k.Wf = static_cast<float>(cur->width);
    k.Hf = static_cast<float>(cur->height);
    k.hw = k.Hf / k.Wf;
    k.cur = camera_consts(*cur);
    k.prev = camera_consts(*prev);
    return k;
}

hipError_t temporal_launch(const mcpt::TemporalParams& k, const TemporalBufs& b, hipStream_t st) {
    auto f4 = [](const float* p) { return reinterpret_cast<const float4*>(p); };
    return mcpt::launch_temporal(k, f4(b.color), f4(b.var), f4(b.albedo_cov), f4(b.normal_depth), f4(b.hist_color_n),
                                 f4(b.hist_var), f4(b.hist_albedo_cov), f4(b.hist_normal_depth),
                                 reinterpret_cast<float4*>(b.out_color_n), reinterpret_cast<float4*>(b.out_var), st);
}

}  // namespace

extern "C" {

int mcpt_abi_version(void) { return MCPT_ABI_VERSION; }

const char* mcpt_last_error(void) { return g_err.c_str(); }

int mcpt_init(const int32_t* devices, int32_t n) {
    return guarded([&]() -> int {
        if (n < 0 || (n > 0 && !devices)) return fail(MCPT_E_INVALID, "bad device list");
        if (n == 0) {                     // the current device, single-device scenes
            g_devices.clear();
            g_peer_ok = true;
            return MCPT_OK;
        }
        int count = 0;
        HIP_TRY(hipGetDeviceCount(&count));
        for (int i = 0; i < n; ++i)
            if (devices[i] < 0 || devices[i] >= count) return fail(MCPT_E_INVALID, "device ordinal out of range");
        // peer access between every pair of distinct listed devices, so the
        // multi-device gather's hipMemcpyPeerAsync is a direct xGMI DMA (without
        // it the runtime stages the copy through host memory); "already
        // enabled" is success, a pair without peer capability keeps the staged copy
        // (the guard restores the caller's device if a HIP call throws mid-loop)
        DeviceGuard guard;
        bool peer_ok = true;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                if (devices[i] == devices[j]) continue;
                int can = 0;
                HIP_TRY(hipDeviceCanAccessPeer(&can, devices[i], devices[j]));
                if (!can) {
                    peer_ok = false;
                    continue;
                }
                HIP_TRY(hipSetDevice(devices[i]));
                const hipError_t e = hipDeviceEnablePeerAccess(devices[j], 0);
                if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
                else HIP_TRY(e);
            }
        g_devices.assign(devices, devices + n);
        g_peer_ok = peer_ok;
        guard.prev = devices[0];          // success: devices[0] becomes current
        return MCPT_OK;
    });
}

int mcpt_device_count(int32_t* out) {
    return guarded([&]() -> int {
        if (!out) return fail(MCPT_E_INVALID, "out is NULL");
        int c = 0;
        HIP_TRY(hipGetDeviceCount(&c));
        *out = c;
        return MCPT_OK;
    });
}

void mcpt_render_params_quinengine(mcpt_render_params* p) {
    if (!p) return;
    mcpt_render_params_default(p);
    p->mode = MCPT_MODE_QUINENGINE;
    p->width = 640; p->height = 480;                 // the QE window (QE/Main.cpp:11, GraphicsRTX.hpp:34-35)
    p->spp = 1;                                       // one sample per pixel per frame (rtx.hlsl:373-404)
    p->max_depth = 5;                                 // sampleMC(..., 5) (rtx.hlsl:400)
    p->illum = 1.0f;                                  // no ILLUM factor
    p->fov_deg = 45.0f;                               // D3DX_PI / 4, vertical (GraphicsRTX.cpp:181)
    p->fresnel_kd = 0;                                // rtx.hlsl:345 (commented out)
    p->seed = 0;                                      // frame seed: the caller's mt19937(1234) draw
}

void mcpt_render_params_default(mcpt_render_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->width = 800; p->height = 600;                 // CV/stdafx.h:41-42
    p->spp = 100;                                     // NUM_SAMPLES_PER_KERNEL
    p->max_depth = 7;                                 // CUTracer.cu:212
    p->illum = 10.0f;                                 // ILLUM
    p->fov_deg = 60.0f;                               // CUTracer.cu:189
    p->eye[0] = 0; p->eye[1] = 5; p->eye[2] = 17;     // scene 1 camera, CUTracer.cu:349-351
    p->dir[0] = 0; p->dir[1] = 0; p->dir[2] = -1;
    p->up[0] = 0; p->up[1] = 1; p->up[2] = 0;
    p->seed = 0x4D435054ull;
    p->fresnel_kd = 1;
    p->tile = 8;
    p->shard_count = 1;
}

void mcpt_denoise_params_default(mcpt_denoise_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->iterations = 5;
    p->normal_power_log2 = 7;
    p->sigma_z = 0.1f;
    p->albedo_floor = 0.01f;
}

void mcpt_denoise_var_params_default(mcpt_denoise_var_params* p) {
    if (!p) return;
    mcpt_denoise_params_default(&p->base);
    p->sigma_l = 4.0f;
}

void mcpt_temporal_params_default(mcpt_temporal_params* p) {
    if (!p) return;
    p->max_history = 32;
    p->normal_threshold = 0.9f;
    p->sigma_z = 0.1f;
    p->gamma_space = 0;
}

void mcpt_adaptive_params_default(mcpt_adaptive_params* p) {
    if (!p) return;
    p->max_passes = 8;
    p->min_passes = 1;
    p->threshold = 0.2f;
    p->lum_floor = 0.01f;
    p->dilate = 1;
    p->force_list = 0;
}

void mcpt_trace_params_default(mcpt_trace_params* p) {
    if (!p) return;
    p->kind = MCPT_TRACE_CLOSEST;
    p->t_max = 0.0f;
    p->lean = 0;
    p->workgroups = 0;
    p->refill = 0;
}

void mcpt_radiance_params_default(mcpt_radiance_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->spp = 1;
    p->max_depth = 7;                                 // CUTracer.cu:212
    p->illum = 10.0f;                                 // ILLUM
    p->fresnel_kd = 1;
    p->seed = 0x4D435054ull;                          // mcpt_render_params_default's
}

void mcpt_ao_params_default(mcpt_ao_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);                     // radius unbounded, bias 0.01, everything else automatic
    p->spp = 1;
    p->seed = 0x4D435054ull;                          // mcpt_render_params_default's
}

void mcpt_direct_params_default(mcpt_direct_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);                     // one chunk, bias 0.01, everything else automatic
    p->spp = 1;
    p->illum = 10.0f;                                 // mcpt_render_params_default's
    p->seed = 0x4D435054ull;
}

// the scene's light table (built at creation, host-only scenes too)
int mcpt_scene_lights(const mcpt_scene* s, int32_t* kd_ids, float* cdf, float* normals, float* area_total) {
    if (!s) return 0;
    const mcpt::LightTable& t = s->lights;
    const size_t L = t.kd_ids.size();
    if (kd_ids && L) std::memcpy(kd_ids, t.kd_ids.data(), L * 4);
    if (cdf && L) std::memcpy(cdf, t.cdf.data(), L * 4);
    if (normals && L) std::memcpy(normals, t.normals.data(), L * 12);
    if (area_total) *area_total = t.area_total;
    return static_cast<int>(L);
}

void mcpt_radiance_ex_params_default(mcpt_radiance_ex_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);                     // the megakernel; every wavefront field automatic
    mcpt_radiance_params_default(&p->base);
}

int mcpt_denoise_device(const mcpt_denoise_params* p, const float* d_color_rgba, const float* d_albedo_cov,
                        const float* d_normal_depth, float* d_out_rgba, float* d_scratch_rgba, void* hip_stream) {
    return guarded([&]() -> int {
        if (!p || !d_color_rgba || !d_albedo_cov || !d_normal_depth || !d_out_rgba || !d_scratch_rgba)
            return fail(MCPT_E_INVALID, "NULL argument");
        mcpt::DenoiseVarParams d{};
        d.base = denoise_resolve(p);
        return denoise_on_device(d, d_color_rgba, nullptr, d_albedo_cov, d_normal_depth, d_out_rgba, d_scratch_rgba,
                                 static_cast<hipStream_t>(hip_stream));
    });
}

int mcpt_denoise(const mcpt_denoise_params* p, const float* color_rgb, const float* albedo_cov,
                 const float* normal_depth, float* out_rgb) {
    return guarded([&]() -> int {
        if (!p || !color_rgb || !albedo_cov || !normal_depth || !out_rgb) return fail(MCPT_E_INVALID, "NULL argument");
        mcpt::DenoiseVarParams d{};
        d.base = denoise_resolve(p);
        return denoise_on_host(d, color_rgb, nullptr, albedo_cov, normal_depth, out_rgb);
    });
}

int mcpt_denoise_var_device(const mcpt_denoise_var_params* p, const float* d_color_rgba, const float* d_var_rgba,
                            const float* d_albedo_cov, const float* d_normal_depth, float* d_out_rgba,
                            float* d_scratch_rgba, void* hip_stream) {
    return guarded([&]() -> int {
        if (!p || !d_color_rgba || !d_var_rgba || !d_albedo_cov || !d_normal_depth || !d_out_rgba || !d_scratch_rgba)
            return fail(MCPT_E_INVALID, "NULL argument");
        return denoise_on_device(denoise_var_resolve(p), d_color_rgba, d_var_rgba, d_albedo_cov, d_normal_depth,
                                 d_out_rgba, d_scratch_rgba, static_cast<hipStream_t>(hip_stream));
    });
}

int mcpt_denoise_var(const mcpt_denoise_var_params* p, const float* color_rgb, const float* var_rgba,
                     const float* albedo_cov, const float* normal_depth, float* out_rgb) {
    return guarded([&]() -> int {
        if (!p || !color_rgb || !var_rgba || !albedo_cov || !normal_depth || !out_rgb)
            return fail(MCPT_E_INVALID, "NULL argument");
        return denoise_on_host(denoise_var_resolve(p), color_rgb, var_rgba, albedo_cov, normal_depth, out_rgb);
    });
}

int mcpt_temporal_device(const mcpt_temporal_params* tp, const mcpt_render_params* cur, const mcpt_render_params* prev,
                         const float* d_color_rgba, const float* d_var_rgba, const float* d_albedo_cov,
                         const float* d_normal_depth, const float* d_hist_color_n, const float* d_hist_var,
                         const float* d_hist_albedo_cov, const float* d_hist_normal_depth, float* d_out_color_n,
                         float* d_out_var, void* hip_stream) {
    return guarded([&]() -> int {
        const TemporalBufs b{d_color_rgba, d_var_rgba, d_albedo_cov, d_normal_depth, d_hist_color_n, d_hist_var,
                             d_hist_albedo_cov, d_hist_normal_depth, d_out_color_n, d_out_var};
        const mcpt::TemporalParams k = temporal_resolve(tp, cur, prev, b);
        HIP_TRY(temporal_launch(k, b, static_cast<hipStream_t>(hip_stream)));
        return MCPT_OK;
    });
}

int mcpt_temporal(const mcpt_temporal_params* tp, const mcpt_render_params* cur, const mcpt_render_params* prev,
                  const float* color_rgba, const float* var_rgba, const float* albedo_cov, const float* normal_depth,
                  const float* hist_color_n, const float* hist_var, const float* hist_albedo_cov,
                  const float* hist_normal_depth, float* out_color_n, float* out_var) {
    return guarded([&]() -> int {
        const TemporalBufs h{color_rgba, var_rgba, albedo_cov, normal_depth, hist_color_n, hist_var, hist_albedo_cov,
                             hist_normal_depth, out_color_n, out_var};
        const mcpt::TemporalParams k = temporal_resolve(tp, cur, prev, h);
        const size_t bytes = size_t(k.width) * size_t(k.height) * 16, vbytes = var_rgba ? bytes : size_t(0);
        // one allocation: the eight inputs in TemporalBufs' order, then the two outputs
        const auto c = carve({bytes, vbytes, bytes, bytes, bytes, vbytes, bytes, bytes, bytes, vbytes});
        TempDev buf(c.total);
        const float* in[8] = {color_rgba, var_rgba, albedo_cov, normal_depth, hist_color_n, hist_var, hist_albedo_cov,
                              hist_normal_depth};
        for (size_t i = 0; i < 8; ++i)
            if (in[i]) HIP_TRY(hipMemcpy(c.at<float>(buf.p, i), in[i], bytes, hipMemcpyHostToDevice));
        auto dv = [&](size_t i) { return var_rgba ? c.at<float>(buf.p, i) : nullptr; };
        const TemporalBufs d{c.at<float>(buf.p, 0), dv(1), c.at<float>(buf.p, 2), c.at<float>(buf.p, 3),
                             c.at<float>(buf.p, 4), dv(5), c.at<float>(buf.p, 6), c.at<float>(buf.p, 7),
                             c.at<float>(buf.p, 8), dv(9)};
        HIP_TRY(temporal_launch(k, d, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        HIP_TRY(hipMemcpy(out_color_n, d.out_color_n, bytes, hipMemcpyDeviceToHost));
        if (out_var) HIP_TRY(hipMemcpy(out_var, d.out_var, bytes, hipMemcpyDeviceToHost));
        return MCPT_OK;
    });
}

}  // extern "C"

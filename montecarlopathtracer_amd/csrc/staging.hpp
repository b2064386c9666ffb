// staging.hpp -- what the host-array entries of the C ABI share when they stage
// their arrays in one device buffer: the carve arithmetic and the RGB <-> RGBA
// converters.  No HIP dependency: tests/cpp/staging_probe.cpp checks it on the CPU.
#pragma once
#include <cstddef>
#include <cstring>

namespace mcpt::host {

// One buffer carved into K parts of bytes[i] each, in order.  Every part
// starts 16-B aligned (float4 loads); `total` is what the buffer must hold.
template <size_t K>
struct Carved {
    size_t off[K];
    size_t total;
    template <typename T>
    T* at(void* base, size_t i) const {
        return reinterpret_cast<T*>(static_cast<char*>(base) + off[i]);
    }
};
template <size_t K>
Carved<K> carve(const size_t (&bytes)[K]) {
    Carved<K> c;
    size_t at = 0;
    for (size_t i = 0; i < K; ++i) {
        c.off[i] = at;
        at = (at + bytes[i] + 15) & ~size_t(15);
    }
    c.total = at;
    return c;
}

// n RGB pixels widened to RGBA (the padding lane 0) and narrowed back; the
// three colour lanes are copied bit for bit (NaN payloads, -0)
inline void rgb_to_rgba(const float* rgb, size_t n, float* rgba) {
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(rgba + 4 * i, rgb + 3 * i, 12);
        rgba[4 * i + 3] = 0.0f;
    }
}
inline void rgba_to_rgb(const float* rgba, size_t n, float* rgb) {
    for (size_t i = 0; i < n; ++i) std::memcpy(rgb + 3 * i, rgba + 4 * i, 12);
}

}  // namespace mcpt::host

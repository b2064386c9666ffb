// Host staging (csrc/staging.hpp): the carve arithmetic and the RGB <-> RGBA
// converters the host-array entries of the C ABI share.
//  - for the part lists of the nine entries, at n / pixel counts 0, 1, 3, 63, 64,
//    65 and 1000: every carved part is 16-B aligned, inside the total, and
//    overlaps no other part
//  - rgba_to_rgb(rgb_to_rgba(x)) == x bit for bit (NaN payloads, -0 included)
//    and the padding lane is 0
// Prints "ok" or the first failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../montecarlopathtracer_amd/csrc/staging.hpp"

using mcpt::host::carve;

template <size_t K>
static bool check_parts(const char* entry, size_t n, const size_t (&bytes)[K]) {
    const auto c = carve(bytes);
    std::vector<char> buf(c.total + 1);
    for (size_t i = 0; i < K; ++i) {
        const bool ok = c.off[i] % 16 == 0 && c.off[i] + bytes[i] <= c.total &&
                        (i + 1 == K || c.off[i] + bytes[i] <= c.off[i + 1]) &&   // offsets ascend: no part reaches the next
                        c.template at<char>(buf.data(), i) == buf.data() + c.off[i];
        if (!ok) {
            std::printf("%s n=%zu: part %zu at %zu (%zu B) of %zu\n", entry, n, i, c.off[i], bytes[i], c.total);
            return false;
        }
    }
    if (c.total % 16 != 0) {
        std::printf("%s n=%zu: total %zu\n", entry, n, c.total);
        return false;
    }
    return true;
}

int main() {
    for (size_t n : {size_t(0), size_t(1), size_t(3), size_t(63), size_t(64), size_t(65), size_t(1000)}) {
        const size_t px = n * 16;
        bool ok = check_parts("mcpt_render", n, {px, size_t(0)}) &&                       // fb (no variance)
                  check_parts("mcpt_render_var", n, {px, px}) &&                          // fb, var
                  check_parts("mcpt_render_aov", n, {px, px}) &&                          // albedo_cov, normal_depth
                  check_parts("mcpt_render_adaptive", n, {px, px, n * 4}) &&              // fb, var, pass counts
                  check_parts("mcpt_denoise", n, {px, size_t(0), px, px, px, px}) &&      // colour, -, features, out, scratch
                  check_parts("mcpt_denoise_var", n, {px, px, px, px, px, px}) &&         // colour, var, features, out, scratch
                  check_parts("mcpt_occluded", n, {n * 12, n * 12, n * 4, n}) &&          // o, d, t_max, flags
                  check_parts("mcpt_radiance", n, {px, n * 12, n * 12, n * 4}) &&         // out, o, d, stream ids
                  check_parts("mcpt_intersect", n, {n * 12, n * 12, n * 12, n * 4, size_t(64), n * 32 * 16});
        if (!ok) return 1;
    }
    // every float bit pattern class: zeros, denormals, infinities, quiet and signalling NaNs with payloads
    const uint32_t bits[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x807FFFFFu, 0x3F800000u, 0xBF800000u, 0x7F7FFFFFu,
                             0x7F800000u, 0xFF800000u, 0x7FC00000u, 0xFFC00001u, 0x7F800001u, 0xFFBFFFFFu, 0x7FFFFFFFu,
                             0x12345678u, 0xDEADBEEFu, 0x7FA5A5A5u};
    const size_t nb = sizeof bits / sizeof bits[0];
    for (size_t n : {size_t(0), size_t(1), size_t(3), size_t(63), size_t(64), size_t(65), size_t(1000)}) {
        std::vector<uint32_t> src(3 * n + 1), wide(4 * n + 1, 0xFFFFFFFFu), back(3 * n + 1, 0xFFFFFFFFu);
        for (size_t i = 0; i < 3 * n; ++i) src[i] = bits[(i * 7 + n) % nb];
        mcpt::host::rgb_to_rgba(reinterpret_cast<const float*>(src.data()), n, reinterpret_cast<float*>(wide.data()));
        mcpt::host::rgba_to_rgb(reinterpret_cast<const float*>(wide.data()), n, reinterpret_cast<float*>(back.data()));
        for (size_t i = 0; i < n; ++i)
            if (wide[4 * i + 3] != 0u) {
                std::printf("n=%zu pixel %zu: padding lane %08x\n", n, i, wide[4 * i + 3]);
                return 1;
            }
        if (std::memcmp(src.data(), back.data(), 3 * n * 4) != 0) {
            std::printf("n=%zu: round trip differs\n", n);
            return 1;
        }
        if (wide[4 * n] != 0xFFFFFFFFu || back[3 * n] != 0xFFFFFFFFu) {   // nothing written past n pixels
            std::printf("n=%zu: wrote past the end\n", n);
            return 1;
        }
    }
    std::printf("ok\n");
    return 0;
}

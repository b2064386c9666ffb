// The sphere clip's host builder (csrc/host_model.cpp clip_spheres, behind
// miss_cull_boxes and direct_list_assign) over hand-made triangle sets, for
// tests/test_sphere_clip_cpu.py, which builds this file with host_model.cpp and
// kd_cache.cpp under AddressSanitizer + UndefinedBehaviorSanitizer and reads:
//   S name boxes=N mask=M             one line per set
//   B name i tris=T sphere=cx cy cz r2   one line per box
// Sets: a tessellated ball beside a wall and a light; a flat strip in place of the
// ball; nothing; one triangle; a ball with a NaN vertex; a ball with huge
// coordinates; a box budget of one; an assignment vector of the wrong length.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../montecarlopathtracer_amd/csrc/host_model.hpp"

namespace {

constexpr int kBoxes = 8;
constexpr double kMargin = 1.0 / 1024.0, kReach = 256.0;

void tri(std::vector<float>& v, const float* a, const float* b, const float* c) {
    for (const float* p : {a, b, c})
        for (int k = 0; k < 3; k++) v.push_back(p[k]);
}

void quad(std::vector<float>& v, const float (&q)[4][3]) {
    tri(v, q[0], q[1], q[2]);
    tri(v, q[0], q[2], q[3]);
}

void ball(std::vector<float>& v, float cx, float cy, float cz, float r, int slices, int stacks) {
    const double pi = 3.14159265358979323846;
    auto at = [&](int i, int j, float* p) {
        const double th = pi * i / stacks, ph = 2.0 * pi * (j % slices) / slices;
        p[0] = cx + r * float(std::sin(th) * std::cos(ph));
        p[1] = cy + r * float(std::cos(th));
        p[2] = cz + r * float(std::sin(th) * std::sin(ph));
    };
    for (int i = 0; i < stacks; i++)
        for (int j = 0; j < slices; j++) {
            float a[3], b[3], c[3], d[3];
            at(i, j, a); at(i, j + 1, b); at(i + 1, j + 1, c); at(i + 1, j, d);
            if (i > 0) tri(v, a, b, c);
            if (i + 1 < stacks) tri(v, a, c, d);
        }
}

void room(std::vector<float>& v) {
    const float wall[4][3] = {{-6, 0, -6}, {6, 0, -6}, {6, 8, -6}, {-6, 8, -6}};
    const float light[4][3] = {{-2, 8, -4}, {2, 8, -4}, {2, 8, 0}, {-2, 8, 0}};
    quad(v, wall);
    quad(v, light);
}

void run(const char* name, const std::vector<float>& verts, int max_boxes = kBoxes, bool short_assign = false) {
    mcpt::HostScene hs;
    hs.kd_verts = verts;
    float boxes[kBoxes][6] = {};
    const int n = mcpt::miss_cull_boxes(hs, boxes, max_boxes);
    std::vector<int32_t> tri_box;
    mcpt::direct_list_assign(hs, boxes, n, tri_box);
    uint32_t count[kBoxes] = {}, want = 0;
    for (int32_t b : tri_box)
        if (b >= 0) count[b]++;
    for (int b = 0; b < n; b++)
        if (count[b] > 2) want |= 1u << b;
    if (short_assign && !tri_box.empty()) tri_box.pop_back();
    float sp[kBoxes][4];
    const uint32_t mask = mcpt::clip_spheres(hs, boxes, n, tri_box, want, kMargin, kReach, sp);
    std::printf("S %s boxes=%d mask=%u\n", name, n, mask);
    for (int b = 0; b < n; b++)
        std::printf("B %s %d tris=%u sphere=%.9g %.9g %.9g %.9g\n", name, b, count[b], sp[b][0], sp[b][1], sp[b][2], sp[b][3]);
}

}  // namespace

int main() {
    std::vector<float> v;
    ball(v, 0, 3, 0, 2, 8, 7);
    room(v);
    run("ball", v);
    run("one_box", v, 1);
    run("short_assign", v, kBoxes, true);
    std::vector<float> w = v;
    w[4] = NAN;
    run("nan_vertex", w);
    w = v;
    for (float& x : w) x *= 1e30f;
    run("huge", w);
    v.clear();
    for (int i = 0; i < 6; i++) {
        const float x0 = -5.0f + 10.0f * i / 6, x1 = -5.0f + 10.0f * (i + 1) / 6;
        const float q[4][3] = {{x0, 1, -1}, {x0, 1, 1}, {x1, 1, 1}, {x1, 1, -1}};
        quad(v, q);
    }
    room(v);
    run("ribbon", v);
    run("nothing", {});
    run("one_triangle", {0, 0, 0, 1, 0, 0, 0, 1, 0});
    return 0;
}

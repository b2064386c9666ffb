/* price_miss_cull.c -- prices the miss cull (render_launch.hpp "Miss cull")
 * on the oracle's own path loop, with no GPU: for every secondary ray of a
 * render, by depth -- does it miss, does it fail every occluder box (the
 * slab test of trace_device.hpp may_hit_scene, in float), did a box-failing
 * ray have a hit after all (must be 0), and what the ordered walk spent on it
 * (inner visits, triangle tests).
 *
 * Diagnostic infrastructure only: it compiles the oracle (oracle/render_ref.c)
 * with its ORC_DIAG_* hooks defined, as scripts/price_descent.c does;
 * scripts/price_miss_cull.py builds and drives it.                          */
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct {
    float o[3], d[3];
    uint64_t inner0, tests0;
} diag_ray;

#define ORC_DIAG_FIELDS diag_ray dg;
/* (expands inside isect_kd_ordered, where the ray is `o`, `d`) */
#define ORC_DIAG_RAY_BEGIN(q) \
    do { (q)->dg.o[0] = o.x; (q)->dg.o[1] = o.y; (q)->dg.o[2] = o.z; (q)->dg.d[0] = d.x; (q)->dg.d[1] = d.y; \
         (q)->dg.d[2] = d.z; (q)->dg.inner0 = (q)->c.inner_visits; (q)->dg.tests0 = (q)->c.tri_tests; } while (0)
#define ORC_DIAG_INNER(q, node) do { } while (0)
#define ORC_DIAG_LEAF(q, node) do { } while (0)
#define ORC_DIAG_POP(q) do { } while (0)
#define ORC_DIAG_ACCEPT(q, node) do { } while (0)
/* (expands inside sample_mc, where the closest hit is `hit`) */
#define ORC_DIAG_AFTER_ISECT(q, depth) diag_after_impl((void*)(q), depth, hit.tri)

static void diag_after_impl(void* q, int depth, int tri);

#include "render_ref.c"

#define DIAG_MAXD 16
static float g_box[16][6];
static int g_nbox;
/* per depth: rays, misses, box failures, box failures with a hit, inner / tests of all rays, of box-failing rays */
static double g_acc[DIAG_MAXD][8];

void diag_init(const float* boxes, int n) {
    g_nbox = n > 16 ? 16 : n;
    memcpy(g_box, boxes, sizeof(float) * 6 * (size_t)g_nbox);
    memset(g_acc, 0, sizeof g_acc);
}

static int may_hit_scene(const float* o, const float* d, float best) {
    for (int b = 0; b < g_nbox; b++) {
        float lo = 0.0f, hi = best;
        for (int a = 0; a < 3; a++) {
            const float inv = 1.0f / d[a];
            const int neg = signbit(d[a]) != 0;
            const float t0 = ((neg ? g_box[b][3 + a] : g_box[b][a]) - o[a]) * inv;
            const float t1 = ((neg ? g_box[b][a] : g_box[b][3 + a]) - o[a]) * inv;
            lo = fmaxf(lo, t0);   /* NaN-passing, as v_max_f32 / v_min_f32 */
            hi = fminf(hi, t1);
        }
        if (!(lo * KD_EPS_LO > hi * KD_EPS_HI)) return 1;
    }
    return 0;
}

static void diag_after_impl(void* qv, int depth, int tri) {
    qctx* q = (qctx*)qv;
    if (depth == 0 || depth >= DIAG_MAXD) return;   /* primary rays are not tested */
    double* a = g_acc[depth];
    const double inner = (double)(q->c.inner_visits - q->dg.inner0), tests = (double)(q->c.tri_tests - q->dg.tests0);
    const int fail = !may_hit_scene(q->dg.o, q->dg.d, q->best_init);
    a[0] += 1;
    a[1] += tri < 0;
    a[2] += fail;
    a[3] += fail && tri >= 0;
    a[4] += inner;
    a[5] += tests;
    if (fail) { a[6] += inner; a[7] += tests; }
}

void diag_read(double* out) { memcpy(out, g_acc, sizeof g_acc); }

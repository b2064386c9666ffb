/* price_direct_lists.c -- prices the direct lists (render_launch.hpp
 * "Direct lists") on the oracle's own path loop, with no GPU: for every
 * secondary ray of a render, by depth -- does its segment hit an occluder box
 * at all (the rays the extend still walks after the miss cull), does it hit
 * exactly one box and a listed one (a direct ray: the slab test of
 * trace_device.hpp scene_box_hits, in float), what the ordered walk spent on
 * it (inner visits, triangle tests), and whether the closest hit over the
 * box's list alone (the oracle's own triangle test, ties by rank) is the
 * walk's hit id (every difference is counted; there must be none).
 *
 * Diagnostic infrastructure only: it compiles the oracle (oracle/render_ref.c)
 * with its ORC_DIAG_* hooks defined, as scripts/price_miss_cull.c does;
 * scripts/price_direct_lists.py builds and drives it.                        */
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
#define DIAG_MAXK 16
static float g_box[16][6];
static int g_nbox;
static int g_cnt[16];                 /* triangles of box b's list, 0 = not listed */
static int g_list[16][DIAG_MAXK];     /* their kd ids */
/* per depth: rays, walked (>= 1 box), direct, direct with another hit id than the walk's,
 * inner / tests of the walked rays, inner / tests of the direct rays */
static double g_acc[DIAG_MAXD][8];

void diag_init(const float* boxes, int n, const int* counts, const int* lists, int k) {
    g_nbox = n > 16 ? 16 : n;
    memcpy(g_box, boxes, sizeof(float) * 6 * (size_t)g_nbox);
    memset(g_cnt, 0, sizeof g_cnt);
    for (int b = 0; b < g_nbox; b++) {
        g_cnt[b] = counts[b] <= DIAG_MAXK ? counts[b] : 0;
        for (int j = 0; j < g_cnt[b]; j++) g_list[b][j] = lists[b * k + j];
    }
    memset(g_acc, 0, sizeof g_acc);
}

static int diag_box_hit(int b, const float* o, const float* d, float best) {
    float lo = 0.0f, hi = best;
    for (int a = 0; a < 3; a++) {
        const float inv = 1.0f / d[a];
        const int neg = signbit(d[a]) != 0;
        const float t0 = ((neg ? g_box[b][3 + a] : g_box[b][a]) - o[a]) * inv;
        const float t1 = ((neg ? g_box[b][a] : g_box[b][3 + a]) - o[a]) * inv;
        lo = fmaxf(lo, t0);   /* NaN-passing, as v_max_f32 / v_min_f32 */
        hi = fminf(hi, t1);
    }
    return !(lo * KD_EPS_LO > hi * KD_EPS_HI);
}

static void diag_after_impl(void* qv, int depth, int tri) {
    qctx* q = (qctx*)qv;
    if (depth == 0 || depth >= DIAG_MAXD) return;   /* primary rays carry no selector */
    double* a = g_acc[depth];
    const double inner = (double)(q->c.inner_visits - q->dg.inner0), tests = (double)(q->c.tri_tests - q->dg.tests0);
    int nh = 0, which = 0;
    for (int b = 0; b < g_nbox; b++)
        if (diag_box_hit(b, q->dg.o, q->dg.d, q->best_init)) { nh++; which = b; }
    a[0] += 1;
    if (!nh) return;                                /* the miss cull's */
    a[1] += 1;
    a[4] += inner;
    a[5] += tests;
    if (nh != 1 || !g_cnt[which]) return;
    a[2] += 1;
    a[6] += inner;
    a[7] += tests;
    const orc_scene* s = q->s;
    const orc_v3 o = {q->dg.o[0], q->dg.o[1], q->dg.o[2]}, d = {q->dg.d[0], q->dg.d[1], q->dg.d[2]};
    hit_t h;
    memset(&h, 0, sizeof h);
    h.tri = -1;
    float best = q->best_init;
    uint32_t bp = 0xFFFFFFFFu;
    for (int j = 0; j < g_cnt[which]; j++) {
        const int k = g_list[which][j];
        tri_test(q->kv[k], o, d, &best, &h, k, s->tri_geom[s->kd_tris[k]], s->kd_prio[k], &bp);
    }
    a[3] += h.tri != tri;
}

void diag_read(double* out) { memcpy(out, g_acc, sizeof g_acc); }

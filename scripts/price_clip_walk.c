/* price_clip_walk.c -- prices the clip walk (render_launch.hpp "Clip walk")
 * on the oracle's own path loop, with no GPU: for every secondary ray of a
 * render -- the mask of the occluder boxes its segment hits (the slab test of
 * trace_device.hpp scene_box_hits, in float), whether the miss cull takes it
 * (no box), the direct resolve (one box, a listed one) or the walk; of the
 * walked rays, which carry a selector (at least one box without a list, at most
 * one with a list) and what the ordered walk spent on them (inner visits,
 * triangle tests), by mask.  For every selected ray the clipped walk is run
 * too: the same ordered walk from the root with the root interval cut to
 * [min lo * KD_EPS_LO, max hi * KD_EPS_HI] over the selector's unlisted boxes --
 * its inner visits and tests, the steps of its single-child prefix (before the
 * first push or leaf: what a start below the root could save at most), whether
 * it finds a hit and, if so, whether that is the walk's hit id; then the listed
 * box's triangles are tested on top, and the result must be the walk's hit id
 * for every ray (both kinds of difference are counted; there must be none).
 *
 * Diagnostic infrastructure only: it compiles the oracle (oracle/render_ref.c)
 * with its ORC_DIAG_* hooks defined, as scripts/price_direct_lists.c does;
 * scripts/price_clip_walk.py builds and drives it.                           */
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

#define DIAG_MAXK 16
enum { A_SECONDARY, A_NOBOX, A_DIRECT, A_WALKED, A_WALK_INNER, A_WALK_TESTS, A_SEL, A_SEL_INNER, A_SEL_TESTS,
       A_CLIP_INNER, A_CLIP_TESTS, A_CLIP_PREFIX, A_CLIP_HITS, A_CLIP_HIT_DIFF, A_FINAL_DIFF, A_EMPTY, A_N };
static float g_box[8][6];
static int g_nbox;
static int g_cnt[8];                  /* triangles of box b's list, 0 = not listed */
static int g_list[8][DIAG_MAXK];      /* their kd ids */
static double g_acc[A_N];
static double g_pat[256][3];          /* by mask, selected rays: rays, inner visits, triangle tests of the full walk */

void diag_init(const float* boxes, int n, const int* counts, const int* lists, int k) {
    g_nbox = n > 8 ? 8 : n;
    memcpy(g_box, boxes, sizeof(float) * 6 * (size_t)g_nbox);
    memset(g_cnt, 0, sizeof g_cnt);
    for (int b = 0; b < g_nbox; b++) {
        g_cnt[b] = counts[b] <= DIAG_MAXK ? counts[b] : 0;
        for (int j = 0; j < g_cnt[b]; j++) g_list[b][j] = lists[b * k + j];
    }
    memset(g_acc, 0, sizeof g_acc);
    memset(g_pat, 0, sizeof g_pat);
}

static int diag_box(int b, const float* o, const float* d, float best, float* plo, float* phi) {
    float lo = 0.0f, hi = best;
    for (int a = 0; a < 3; a++) {
        const float inv = 1.0f / d[a];
        const int neg = signbit(d[a]) != 0;
        const float t0 = ((neg ? g_box[b][3 + a] : g_box[b][a]) - o[a]) * inv;
        const float t1 = ((neg ? g_box[b][a] : g_box[b][3 + a]) - o[a]) * inv;
        lo = fmaxf(lo, t0);   /* NaN-passing, as v_max_f32 / v_min_f32 */
        hi = fminf(hi, t1);
    }
    *plo = lo;
    *phi = hi;
    return !(lo * KD_EPS_LO > hi * KD_EPS_HI);
}

/* isect_kd_ordered (no child boxes) with the root interval cut to [clo, chi]; its own counters */
static hit_t clip_walk(qctx* q, orc_v3 o, orc_v3 d, float clo, float chi, float* pbest, uint32_t* pprio,
                       double* inner, double* tests, double* prefix) {
    const orc_scene* s = q->s;
    hit_t h;
    memset(&h, 0, sizeof h);
    h.tri = -1; h.geom = -1;
    float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    float inv[3] = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    const orc_node* root = &s->nodes[0];
    float tmin = 0.0f, tmax = FLT_MAX;
    for (int a = 0; a < 3; a++) {
        if (dd[a] == 0.0f) {
            if (oo[a] < root->bmin[a] || oo[a] > root->bmax[a]) return h;
        } else {
            float t0 = (root->bmin[a] - oo[a]) * inv[a];
            float t1 = (root->bmax[a] - oo[a]) * inv[a];
            float lo = dd[a] < 0.0f ? t1 : t0;
            float hi = dd[a] < 0.0f ? t0 : t1;
            tmin = lo > tmin ? lo : tmin;
            tmax = hi < tmax ? hi : tmax;
        }
    }
    tmin = clo > tmin ? clo : tmin;
    tmax = chi < tmax ? chi : tmax;
    if (tmin > tmax * KD_EPS_HI) { g_acc[A_EMPTY] += 1; return h; }
    uint32_t st_node[40];
    float st_lo[40], st_hi[40];
    int sp = 0, in_prefix = 1;
    uint32_t node = 0;
    for (;;) {
        const orc_node* nd = &s->nodes[node];
        while (nd->axis) {
            *inner += 1;
            int a = (int)nd->axis - 1;
            float sv = nd->split;
            float t = (sv - oo[a]) * inv[a];
            int below = (oo[a] < sv) || (oo[a] == sv && dd[a] <= 0.0f);
            uint32_t nearc = below ? nd->left : nd->right;
            uint32_t farc = below ? nd->right : nd->left;
            if (dd[a] == 0.0f && oo[a] == sv) {
                st_node[sp] = farc; st_lo[sp] = tmin; st_hi[sp] = tmax; sp++;
                node = nearc;
                in_prefix = 0;
            } else if (!(t > 0.0f) || t > tmax * KD_EPS_HI) {
                node = nearc;
            } else if (t * KD_EPS_HI < tmin) {
                node = farc;
            } else {
                st_node[sp] = farc; st_lo[sp] = t > tmin ? t : tmin; st_hi[sp] = tmax; sp++;
                node = nearc;
                tmax = t < tmax ? t : tmax;
                in_prefix = 0;
            }
            *prefix += in_prefix;
            nd = &s->nodes[node];
        }
        in_prefix = 0;
        for (uint32_t i = 0; i < nd->tri_count; i++) {
            uint32_t k = s->leaf_ids[nd->tri_begin + i];
            *tests += 1;
            tri_test(q->kv[k], o, d, pbest, &h, (int)k, s->tri_geom[s->kd_tris[k]], s->kd_prio[k], pprio);
        }
        if (sp == 0) break;
        sp--;
        node = st_node[sp]; tmin = st_lo[sp]; tmax = st_hi[sp];
        if (*pbest <= tmin * KD_EPS_LO) break;
    }
    return h;
}

static void diag_after_impl(void* qv, int depth, int tri) {
    qctx* q = (qctx*)qv;
    if (depth == 0) return;                         /* primary rays carry no selector */
    const double inner = (double)(q->c.inner_visits - q->dg.inner0), tests = (double)(q->c.tri_tests - q->dg.tests0);
    int mask = 0, nl = 0, nu = 0, lbox = -1;
    float clo = FLT_MAX, chi = 0.0f;
    for (int b = 0; b < g_nbox; b++) {
        float lo, hi;
        if (!diag_box(b, q->dg.o, q->dg.d, q->best_init, &lo, &hi)) continue;
        mask |= 1 << b;
        if (g_cnt[b]) { nl++; lbox = b; }
        else { nu++; clo = fminf(clo, lo); chi = fmaxf(chi, hi); }
    }
    g_acc[A_SECONDARY] += 1;
    if (!mask) { g_acc[A_NOBOX] += 1; return; }     /* the miss cull's */
    if (nl == 1 && nu == 0) { g_acc[A_DIRECT] += 1; return; }   /* the direct resolve's */
    g_acc[A_WALKED] += 1;
    g_acc[A_WALK_INNER] += inner;
    g_acc[A_WALK_TESTS] += tests;
    if (nu < 1 || nl > 1) return;                   /* the full walk */
    g_acc[A_SEL] += 1;
    g_acc[A_SEL_INNER] += inner;
    g_acc[A_SEL_TESTS] += tests;
    g_pat[mask][0] += 1;
    g_pat[mask][1] += inner;
    g_pat[mask][2] += tests;
    const orc_scene* s = q->s;
    const orc_v3 o = {q->dg.o[0], q->dg.o[1], q->dg.o[2]}, d = {q->dg.d[0], q->dg.d[1], q->dg.d[2]};
    float best = q->best_init;
    uint32_t bp = 0xFFFFFFFFu;
    hit_t h = clip_walk(q, o, d, clo * KD_EPS_LO, chi * KD_EPS_HI, &best, &bp, &g_acc[A_CLIP_INNER], &g_acc[A_CLIP_TESTS],
                        &g_acc[A_CLIP_PREFIX]);
    if (h.tri >= 0) {
        g_acc[A_CLIP_HITS] += 1;
        g_acc[A_CLIP_HIT_DIFF] += h.tri != tri;
    }
    for (int j = 0; lbox >= 0 && j < g_cnt[lbox]; j++) {
        const int k = g_list[lbox][j];
        tri_test(q->kv[k], o, d, &best, &h, k, s->tri_geom[s->kd_tris[k]], s->kd_prio[k], &bp);
    }
    g_acc[A_FINAL_DIFF] += h.tri != tri;
}

void diag_read(double* acc, double* pat) {
    memcpy(acc, g_acc, sizeof g_acc);
    memcpy(pat, g_pat, sizeof g_pat);
}
int diag_nacc(void) { return A_N; }

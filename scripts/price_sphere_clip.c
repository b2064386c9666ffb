/* price_sphere_clip.c -- prices the sphere clip (render_launch.hpp "Sphere clip")
 * on the oracle's own path loop, with no GPU, beside the clip walk it refines
 * (scripts/price_clip_walk.c, whose selector and clipped walk are restated here).
 * For every secondary ray that reaches an extend with a selector -- a ray made for
 * the terminal query that can reach no emitter box is dropped first, as the shade
 * drops it -- three walks are compared: the full ordered walk (the oracle's), the
 * clipped walk (root interval cut to the union of the selector's unlisted boxes'
 * slab intervals) and the sphere-clipped walk (each such box's interval first cut
 * to the ray's interval in that box's sphere, wf_extend_body.hpp's start-up in
 * float, operation for operation: compile with -ffp-contract=off).  Counted: inner
 * visits and triangle tests of each, the walks the spheres leave nothing of (the
 * device's sphere_skips), and the rays whose hit id -- the walk's, with the listed
 * box's triangles tested on top -- differs from the full walk's (must be 0).
 *
 * diag_rays runs the restated clipped walk plus list over a batch of rays with
 * intervals the caller computed (tests/test_sphere_clip_cpu.py: numpy's).
 *
 * Diagnostic infrastructure only: it compiles the oracle (oracle/render_ref.c)
 * with its ORC_DIAG_* hooks defined; scripts/price_sphere_clip.py drives it.   */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
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
enum { A_SECONDARY, A_TERMINAL_CULLED, A_SEL, A_FULL_INNER, A_FULL_TESTS, A_CLIP_INNER, A_CLIP_TESTS, A_CLIP_EMPTY,
       A_SPH_INNER, A_SPH_TESTS, A_SPH_EMPTY, A_SKIPS, A_CLIP_DIFF, A_SPH_DIFF, A_N };
static float g_box[8][6];
static int g_nbox;
static int g_cnt[8];                  /* triangles of box b's list, 0 = not listed */
static int g_list[8][DIAG_MAXK];      /* their kd ids */
static int g_sphmask;                 /* bit b: box b has a sphere */
static float g_sph[8][4];             /* {centre xyz, radius^2} */
static float g_cull[8][6];            /* the terminal cull's emitter boxes as the device decodes them */
static int g_ncull, g_terminal;       /* g_terminal: the terminal query's depth, < 0: no terminal cull */
static double g_acc[A_N];

/* terminal: the terminal query's depth (the render's max_depth) where the scene allows the terminal cull,
 * else < 0; the emitter boxes are taken from the scene as the product takes them (one box per emitter
 * geometry over its triangles' vertices, rounded outward to binary16) */
void diag_init(const orc_scene* s, const float* boxes, int n, const int* counts, const int* lists, int k, int sphmask,
               const float* spheres, int terminal) {
    g_nbox = n > 8 ? 8 : n;
    memcpy(g_box, boxes, sizeof(float) * 6 * (size_t)g_nbox);
    memset(g_cnt, 0, sizeof g_cnt);
    for (int b = 0; b < g_nbox; b++) {
        g_cnt[b] = counts[b] <= DIAG_MAXK ? counts[b] : 0;
        for (int j = 0; j < g_cnt[b]; j++) g_list[b][j] = lists[b * k + j];
    }
    g_sphmask = sphmask;
    memcpy(g_sph, spheres, sizeof g_sph);
    g_ncull = 0;
    for (int g = 0; g < s->ngeoms && g_ncull < 8; g++) {
        if (!(s->geoms[g].Ka.x > 0 || s->geoms[g].Ka.y > 0 || s->geoms[g].Ka.z > 0)) continue;
        float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        for (int i = 0; i < s->model.ntris; i++) {
            if (s->tri_geom[i] != g) continue;
            for (int j = 0; j < 3; j++) {
                const orc_v3 p = s->model.verts[s->model.tris[i].v[j]];
                const float c[3] = {p.x, p.y, p.z};
                for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], c[a]); hi[a] = fmaxf(hi[a], c[a]); }
            }
        }
        for (int a = 0; a < 3; a++) {
            g_cull[g_ncull][a] = orc_f16_to_f32(orc_f16_dir(lo[a], -1));
            g_cull[g_ncull][3 + a] = orc_f16_to_f32(orc_f16_dir(hi[a], +1));
        }
        g_ncull++;
    }
    g_terminal = g_ncull ? terminal : -1;
    memset(g_acc, 0, sizeof g_acc);
}

/* trace_device.hpp box_interval / slab_hit on fp32 bounds */
static int slab(const float* bx, const float* o, const float* d, float best, float* plo, float* phi) {
    float lo = 0.0f, hi = best;
    for (int a = 0; a < 3; a++) {
        const float inv = 1.0f / d[a];
        const int neg = signbit(d[a]) != 0;
        const float t0 = ((neg ? bx[3 + a] : bx[a]) - o[a]) * inv;
        const float t1 = ((neg ? bx[a] : bx[3 + a]) - o[a]) * inv;
        lo = fmaxf(lo, t0);   /* NaN-passing, as v_max_f32 / v_min_f32 */
        hi = fminf(hi, t1);
    }
    *plo = lo;
    *phi = hi;
    return !(lo * KD_EPS_LO > hi * KD_EPS_HI);
}

/* trace_device.hpp sphere_interval, then the start-up's "nothing left" rule */
static void sphere_cut(const float* s, const float* o, const float* d, float* plo, float* phi) {
    const float mx = s[0] - o[0], my = s[1] - o[1], mz = s[2] - o[2];
    const float a = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const float b = (mx * d[0] + my * d[1]) + mz * d[2];
    const float ia = 1.0f / a;
    const float tc = b * ia;
    const float px = mx - tc * d[0], py = my - tc * d[1], pz = mz - tc * d[2];
    const float q = s[3] - ((px * px + py * py) + pz * pz);
    const float h = sqrtf(q * ia);
    const int miss = q < 0.0f;
    float lo = miss ? FLT_MAX : fmaxf(*plo, tc - h);
    float hi = miss ? 0.0f : fminf(*phi, tc + h);
    if (lo * KD_EPS_LO > hi * KD_EPS_HI) { lo = FLT_MAX; hi = 0.0f; }
    *plo = lo;
    *phi = hi;
}

/* isect_kd_ordered (no child boxes) with the root interval cut to [clo, chi]; its own counters.
 * *started = 0: the interval was empty at the root (the device's walk == false) */
static hit_t clip_walk(qctx* q, orc_v3 o, orc_v3 d, float clo, float chi, float* pbest, uint32_t* pprio,
                       double* inner, double* tests, int* started) {
    const orc_scene* s = q->s;
    hit_t h;
    memset(&h, 0, sizeof h);
    h.tri = -1; h.geom = -1;
    *started = 0;
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
    if (tmin > tmax * KD_EPS_HI) return h;
    tmin = fmaxf(tmin, clo);          /* (NaN-passing, as the device's) */
    tmax = fminf(tmax, chi);
    if (tmin > tmax * KD_EPS_HI) return h;
    *started = 1;
    uint32_t st_node[40];
    float st_lo[40], st_hi[40];
    int sp = 0;
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
            } else if (!(t > 0.0f) || t > tmax * KD_EPS_HI) {
                node = nearc;
            } else if (t * KD_EPS_HI < tmin) {
                node = farc;
            } else {
                st_node[sp] = farc; st_lo[sp] = t > tmin ? t : tmin; st_hi[sp] = tmax; sp++;
                node = nearc;
                tmax = t < tmax ? t : tmax;
            }
            nd = &s->nodes[node];
        }
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

/* the clipped walk over [clo * KD_EPS_LO, chi * KD_EPS_HI], then box lbox's list on top: the hit id */
static int walk_and_list(qctx* q, orc_v3 o, orc_v3 d, float clo, float chi, int lbox, double* inner, double* tests,
                         int* started) {
    const orc_scene* s = q->s;
    float best = q->best_init;
    uint32_t bp = 0xFFFFFFFFu;
    hit_t h = clip_walk(q, o, d, clo * KD_EPS_LO, chi * KD_EPS_HI, &best, &bp, inner, tests, started);
    for (int j = 0; lbox >= 0 && j < g_cnt[lbox]; j++) {
        const int k = g_list[lbox][j];
        tri_test(q->kv[k], o, d, &best, &h, k, s->tri_geom[s->kd_tris[k]], s->kd_prio[k], &bp);
    }
    return h.tri;
}

static void diag_after_impl(void* qv, int depth, int tri) {
    qctx* q = (qctx*)qv;
    if (depth == 0) return;                         /* primary rays carry no selector */
    const double inner = (double)(q->c.inner_visits - q->dg.inner0), tests = (double)(q->c.tri_tests - q->dg.tests0);
    int mask = 0, nl = 0, nu = 0, lbox = -1;
    float clo = FLT_MAX, chi = 0.0f, slo = FLT_MAX, shi = 0.0f;
    g_acc[A_SECONDARY] += 1;
    for (int b = 0; b < g_nbox; b++) {
        float lo, hi;
        if (!slab(g_box[b], q->dg.o, q->dg.d, q->best_init, &lo, &hi)) continue;
        mask |= 1 << b;
        if (g_cnt[b]) { nl++; lbox = b; continue; }
        nu++;
        clo = fminf(clo, lo); chi = fmaxf(chi, hi);
        if ((g_sphmask >> b) & 1) sphere_cut(g_sph[b], q->dg.o, q->dg.d, &lo, &hi);
        slo = fminf(slo, lo); shi = fmaxf(shi, hi);
    }
    if (!mask) return;                              /* the miss cull's */
    if (nl == 1 && nu == 0) return;                 /* the direct resolve's */
    if (depth == g_terminal) {                      /* the terminal cull, where the shade makes the ray */
        int reach = 0;
        float lo, hi;
        for (int b = 0; b < g_ncull; b++) reach |= slab(g_cull[b], q->dg.o, q->dg.d, q->best_init, &lo, &hi);
        if (!reach) { g_acc[A_TERMINAL_CULLED] += 1; return; }
    }
    if (nu < 1 || nl > 1) return;                   /* the full walk */
    g_acc[A_SEL] += 1;
    g_acc[A_FULL_INNER] += inner;
    g_acc[A_FULL_TESTS] += tests;
    const orc_v3 o = {q->dg.o[0], q->dg.o[1], q->dg.o[2]}, d = {q->dg.d[0], q->dg.d[1], q->dg.d[2]};
    int started_c, started_s;
    const int hc = walk_and_list(q, o, d, clo, chi, lbox, &g_acc[A_CLIP_INNER], &g_acc[A_CLIP_TESTS], &started_c);
    const int hs = walk_and_list(q, o, d, slo, shi, lbox, &g_acc[A_SPH_INNER], &g_acc[A_SPH_TESTS], &started_s);
    g_acc[A_CLIP_EMPTY] += !started_c;
    g_acc[A_SPH_EMPTY] += !started_s;
    g_acc[A_SKIPS] += started_c && !started_s;
    g_acc[A_CLIP_DIFF] += hc != tri;
    g_acc[A_SPH_DIFF] += hs != tri;
}

void diag_read(double* acc) { memcpy(acc, g_acc, sizeof g_acc); }
int diag_nacc(void) { return A_N; }

/* the restated clipped walk plus list over n rays: ray i walks [clo[i] * KD_EPS_LO, chi[i] * KD_EPS_HI]
 * (an empty interval starts no walk), then box lbox[i]'s list (< 0: none) is tested on top */
void diag_rays(const orc_scene* s, int64_t n, const float* o, const float* d, const float* clo, const float* chi,
               const int32_t* lbox, int32_t* tri_out, int32_t* started_out) {
    qctx q;
    memset(&q, 0, sizeof q);
    q.s = s;
    q.best_init = FLT_MAX;
    orc_v3(*kv)[3] = malloc(sizeof(orc_v3[3]) * (size_t)(s->nkd ? s->nkd : 1));
    for (int k = 0; k < s->nkd; k++)
        for (int j = 0; j < 3; j++) kv[k][j] = s->model.verts[s->model.tris[s->kd_tris[k]].v[j]];
    q.kv = (const orc_v3(*)[3])kv;
    double inner = 0, tests = 0;
    for (int64_t i = 0; i < n; i++) {
        int started;
        tri_out[i] = walk_and_list(&q, v3(o[3 * i], o[3 * i + 1], o[3 * i + 2]), v3(d[3 * i], d[3 * i + 1], d[3 * i + 2]),
                                   clo[i], chi[i], lbox[i], &inner, &tests, &started);
        started_out[i] = started;
    }
    free(kv);
}

// Catalogue top-K and ranks over a ReLU-sum: r4r_topk_relu / r4r_pair_relu / r4r_rank_relu (include/r4r.h, "Catalogue
// recommendation: ReLU-sum heads").
//
//   h = fmaf(w[j], fmaxf(q[u][j] + c[i][j], 0), h)   j < H        d = fmaf(q[u][H + j], c[i][H + j], d)   j < P
//   score(u, i) = ((h + d) + c_bias[i]) + q_bias[u]
//
// The ReLU sits inside the sum, so this is no MFMA shape: 3 H + P vector instructions per pair, bound by VALU issue.
// Launch 1, relu_scan_kernel: one WAVE per workgroup = (tile of RELU_QT queries) x (chunk of candidates).  Lane =
// candidate: the wave takes 64 candidates at a time, every lane loads RELU_CB columns of ITS row into registers, and
// the tile's queries walk over that block -- q[u][j] and w[j] are wave-uniform and come from LDS reads at one address
// (the tile's query rows are staged there once, column-major, so a column's RELU_QT values are four ds_read_b128).
// One accumulator per query and chain stays in registers while the columns stream by in blocks.  Scores are never
// written: each is compared with its query's K-th best, survivors go through topk_device.h's list_insert, the partial
// lists have r4r_topk_dot's workspace layout and topk.hip's merge kernel finishes (skipped for a single chunk).
// r4r_rank_relu: the same stream with counters in place of lists.  The two streams and topk_device.h's scalar kernels
// over this file's ReluHead compute a score with the SAME instruction sequence on the same operands (relu_term / the
// fmaf of the dot, ascending j, three additions), so a score's bits depend on its own pair only.
// This file has the two streams and the head; the scalar kernels, the chunk rule, the argument checks and the plan of a
// call are topk_device.h's, shared with topk.hip and topk_hmlp.hip.
#include <math.h>

#include "common.h"
#include "slate_device.h"
#include "topk_device.h"

namespace r4r {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RELU_MAX_H = 128;
constexpr int RELU_MAX_P = 128;
constexpr int RELU_QT = 16;        // queries (pairs, for the rank) per wave
constexpr int RELU_CB = 8;         // columns of a candidate row a lane holds at a time

// one hidden term of the chain: add, max, fma -- explicitly these three
__device__ __forceinline__ float relu_term(float w, float q, float c, float h) {
    return __builtin_fmaf(w, __builtin_fmaxf(q + c, 0.f), h);
}

// the scalar chain of one pair: q, c point at the pair's rows
__device__ __forceinline__ float relu_pair_score(const float *q, const float *c, const float *w, int H, int P, float cb,
                                                 float qb) {
    float h = 0.f, d = 0.f;
    for (int j = 0; j < H; ++j) h = relu_term(w[j], q[j], c[j], h);
    for (int j = 0; j < P; ++j) d = __builtin_fmaf(q[H + j], c[H + j], d);
    return ((h + d) + cb) + qb;
}

// The head of this form (topk_device.h): the scalar chain over the rows of pair (u, i)
struct ReluHead {
    const float *q, *q_bias, *c, *c_bias, *w;
    int64_t n_c, c_stride;
    int H, P;

    __device__ __forceinline__ float q_bias_of(int64_t u) const { return q_bias ? q_bias[u] : 0.f; }
    __device__ __forceinline__ float score(int64_t u, int64_t i, float qb) const {
        return relu_pair_score(q + u * (H + P), c + i * c_stride, w, H, P, c_bias ? c_bias[i] : 0.f, qb);
    }
    __device__ __forceinline__ float score(int64_t u, int64_t i) const { return score(u, i, q_bias_of(u)); }

    static constexpr const char *width_name = "H + P";
    int width() const { return H + P; }
    int ranges(const char *fn) const {
        R4R_REQUIRE(H >= 0 && H <= RELU_MAX_H, "%s: H = %d outside 0 .. %d", fn, H, RELU_MAX_H);
        R4R_REQUIRE(P >= 0 && P <= RELU_MAX_P, "%s: P = %d outside 0 .. %d", fn, P, RELU_MAX_P);
        return R4R_OK;
    }
    int weights(const char *fn) const {
        R4R_REQUIRE(H == 0 || w != nullptr, "%s: null w with H > 0", fn);
        return R4R_OK;
    }
};

inline ReluHead relu_head(const float *q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                          const float *c_bias, const float *w, int H, int P) {
    ReluHead h;
    h.q = q; h.q_bias = q_bias; h.c = c; h.c_bias = c_bias; h.w = w;
    h.n_c = n_c; h.c_stride = c_stride; h.H = H; h.P = P;
    return h;
}

// NB columns from j0 of the lane's candidate row against the tile's queries.  qs: LDS [H + P][RELU_QT] (column-major),
// ws: LDS [H]; both addresses are wave-uniform.
template <int NB>
__device__ __forceinline__ void relu_hidden_block(const float *qs, const float *ws, const float *row, int j0,
                                                  float (&h)[RELU_QT]) {
    float cv[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) cv[k] = row[j0 + k];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const float wj = ws[j0 + k];
        const f32x4 *qv = reinterpret_cast<const f32x4 *>(qs + (size_t)(j0 + k) * RELU_QT);
#pragma unroll
        for (int g = 0; g < RELU_QT / 4; ++g) {
            const f32x4 v = qv[g];
#pragma unroll
            for (int e = 0; e < 4; ++e) h[4 * g + e] = relu_term(wj, v[e], cv[k], h[4 * g + e]);
        }
    }
}

template <int NB>
__device__ __forceinline__ void relu_dot_block(const float *qs, const float *row, int j0, float (&d)[RELU_QT]) {
    float cv[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) cv[k] = row[j0 + k];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const f32x4 *qv = reinterpret_cast<const f32x4 *>(qs + (size_t)(j0 + k) * RELU_QT);
#pragma unroll
        for (int g = 0; g < RELU_QT / 4; ++g) {
            const f32x4 v = qv[g];
#pragma unroll
            for (int e = 0; e < 4; ++e) d[4 * g + e] = __builtin_fmaf(v[e], cv[k], d[4 * g + e]);
        }
    }
}

// the scores of the lane's candidate against the tile's RELU_QT queries; qbs: LDS [RELU_QT]
__device__ __forceinline__ void relu_slab_scores(const float *qs, const float *ws, const float *qbs, const float *row, int H,
                                                 int P, float cb, float (&sv)[RELU_QT]) {
    float h[RELU_QT], d[RELU_QT];
#pragma unroll
    for (int i = 0; i < RELU_QT; ++i) { h[i] = 0.f; d[i] = 0.f; }
    int j = 0;
#pragma unroll 1
    for (; j + RELU_CB <= H; j += RELU_CB) relu_hidden_block<RELU_CB>(qs, ws, row, j, h);
#pragma unroll 1
    for (; j < H; ++j) relu_hidden_block<1>(qs, ws, row, j, h);
    const int HP = H + P;
#pragma unroll 1
    for (; j + RELU_CB <= HP; j += RELU_CB) relu_dot_block<RELU_CB>(qs, row, j, d);
#pragma unroll 1
    for (; j < HP; ++j) relu_dot_block<1>(qs, row, j, d);
#pragma unroll
    for (int g = 0; g < RELU_QT / 4; ++g) {
        const f32x4 b = reinterpret_cast<const f32x4 *>(qbs)[g];
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[4 * g + e] = ((h[4 * g + e] + d[4 * g + e]) + cb) + b[e];
    }
}

struct ReluScanArgs {
    const float *q, *q_bias, *c, *c_bias, *w;
    const int64_t *excl_off, *excl_ids;
    float *out_scores;        // [n_q, parts, K]
    int64_t *out_ids;
    int64_t n_q, n_c, c_stride, chunk, parts, tiles;
    int H, P, K;
};

inline size_t relu_stage_floats(int H, int P) { return (size_t)(H + P) * RELU_QT + (size_t)RELU_QT + (size_t)H; }

__global__ __launch_bounds__(64) void relu_scan_kernel(ReluScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char relu_lds[];
    constexpr int QT = RELU_QT;
    const int K = a.K, H = a.H, P = a.P, HP = H + P;
    float *qs = reinterpret_cast<float *>(relu_lds);           // [HP][QT]
    float *qbs = qs + (size_t)HP * QT;                         // [QT]
    float *ws = qbs + QT;                                      // [H]
    float *sc = ws + H;                                        // [QT][K]
    int *id = reinterpret_cast<int *>(sc + QT * K);            // [QT][K]  candidate - chunk begin

    const int lane = threadIdx.x;
    const ChunkGeom g = chunk_geom(a.tiles, QT, a.chunk, a.n_c);
    const int64_t u0 = g.first, c_begin = g.c_begin, c_end = g.c_end;

    for (int i = lane; i < QT * K; i += 64) { sc[i] = -INFINITY; id[i] = fill_id<int>::value; }
    for (int e = lane; e < HP * QT; e += 64) {
        const int j = e / QT;
        const int64_t u = u0 + (e % QT);
        qs[e] = u < a.n_q ? a.q[u * HP + j] : 0.f;
    }
    if (lane < QT) qbs[lane] = (a.q_bias != nullptr && u0 + lane < a.n_q) ? a.q_bias[u0 + lane] : 0.f;
    for (int j = lane; j < H; j += 64) ws[j] = a.w[j];
    float thr[QT];                                             // the K-th best of each query (wave-uniform)
#pragma unroll
    for (int i = 0; i < QT; ++i) thr[i] = (u0 + i < a.n_q) ? -INFINITY : INFINITY;      // rows past n_q never survive
    wave_lds_fence();

    for (int64_t base = c_begin; base < c_end; base += 64) {
        const int64_t cand = base + lane;
        const bool live = cand < c_end;
        const int64_t ic = cand < a.n_c ? cand : a.n_c - 1;   // a row past the table reads the table's last row
        const float *row = a.c + ic * a.c_stride;              // (never dereferenced when H + P == 0)
        const float cb = a.c_bias != nullptr ? a.c_bias[ic] : 0.f;
        float sv[QT];
        relu_slab_scores(qs, ws, qbs, row, H, P, cb, sv);
        bool any = false;
#pragma unroll
        for (int i = 0; i < QT; ++i) any |= live && sv[i] > thr[i];
        if (__ballot(any) == 0) continue;
        // survivors, one at a time (wave-uniform control flow from here on)
#pragma unroll
        for (int i = 0; i < QT; ++i) {
            unsigned long long m = __ballot(live && sv[i] > thr[i]);
            while (m) {
                const int src = __builtin_ctzll(m);
                m &= m - 1;
                const float v = lane_value(sv[i], src);
                const int64_t ci = base + src;
                if (!(v > thr[i])) continue;                   // (an earlier survivor raised the bar)
                if (is_excluded(a.excl_off, a.excl_ids, u0 + i, ci)) continue;
                thr[i] = list_insert<int>(sc + i * K, id + i * K, K, v, (int)(ci - c_begin), lane);
            }
        }
    }

    // the partial lists, filled up with (-inf, -1)
    for (int ql = 0; ql < QT; ++ql) {
        const int64_t u = u0 + ql;
        if (u >= a.n_q) break;
        const int64_t o = (u * a.parts + g.part) * K;
        for (int p = lane; p < K; p += 64) {
            const int ci = id[ql * K + p];
            a.out_scores[o + p] = sc[ql * K + p];              // (-inf in an unused slot)
            a.out_ids[o + p] = ci != fill_id<int>::value ? c_begin + ci : (int64_t)-1;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// r4r_rank_relu: r4r_rank_dot's three launches over this file's chain.
//   A  rank_target_kernel<ReluHead>   one thread per pair: the scalar chain -> out_score[p]; out_rank[p] = 0, or -1 for
//                                     a target whose own score is -inf or NaN (never touched again)
//   B  rank_relu_scan_kernel          the scan's stream over a tile of RELU_QT PAIRS (query rows gathered through q_idx
//                                     into LDS) and a chunk of candidates; every score is compared with the pair's
//                                     target in registers and counted; one 64-bit integer atomic per (pair, chunk)
//   C  rank_excl_kernel<ReluHead>     only with exclusions: B counted the excluded ids too; one wave per pair recomputes
//                                     the scalar chain of its query row's excluded ids and subtracts those that were ahead
// (A and C: topk_device.h.)
struct ReluRankArgs {
    const float *q, *q_bias, *c, *c_bias, *w;
    const int64_t *q_idx, *t_idx;
    const float *t_score;     // out_score, written by launch A
    int64_t *out_rank;
    int64_t n_p, n_c, c_stride, chunk, tiles;
    int H, P;
};

__global__ __launch_bounds__(64) void rank_relu_scan_kernel(ReluRankArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char relu_lds[];
    constexpr int PT = RELU_QT;
    const int H = a.H, P = a.P, HP = H + P;
    float *qs = reinterpret_cast<float *>(relu_lds);           // [HP][PT]
    float *qbs = qs + (size_t)HP * PT;                         // [PT]
    float *ws = qbs + PT;                                      // [H]

    const int lane = threadIdx.x;
    const ChunkGeom g = chunk_geom(a.tiles, PT, a.chunk, a.n_c);
    const int64_t p0 = g.first, c_begin = g.c_begin, c_end = g.c_end;
    const int c_len = g.c_len();

    for (int e = lane; e < HP * PT; e += 64) {
        const int j = e / PT;
        const int64_t p = p0 + (e % PT);
        qs[e] = p < a.n_p ? a.q[a.q_idx[p] * HP + j] : 0.f;
    }
    if (lane < PT) qbs[lane] = (a.q_bias != nullptr && p0 + lane < a.n_p) ? a.q_bias[a.q_idx[p0 + lane]] : 0.f;
    for (int j = lane; j < H; j += 64) ws[j] = a.w[j];
    // Of each pair: its target's score and its target's id relative to the chunk (-1: before it, so no tie is ahead;
    // INT_MAX: behind it, so every tie is).  A pair past n_p or at -1 waits for a score above +inf: it counts nothing.
    float ts[PT];
    int trel[PT], cnt[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        const int64_t p = p0 + i;
        const int64_t pc = p < a.n_p ? p : a.n_p - 1;
        const float st = a.t_score[pc];
        const int64_t d = a.t_idx[pc] - c_begin;
        const bool ranked = p < a.n_p && st > -INFINITY;       // (false for NaN)
        ts[i] = ranked ? st : INFINITY;
        trel[i] = !ranked || d < 0 ? -1 : (d > 0x7fffffff ? 0x7fffffff : (int)d);
        cnt[i] = 0;
    }
    wave_lds_fence();

    for (int64_t base = c_begin; base < c_end; base += 64) {
        const int rel = (int)(base - c_begin) + lane;
        const bool live = rel < c_len;
        const int64_t cand = base + lane;
        const int64_t ic = cand < a.n_c ? cand : a.n_c - 1;
        const float *row = a.c + ic * a.c_stride;
        const float cb = a.c_bias != nullptr ? a.c_bias[ic] : 0.f;
        float sv[PT];
        relu_slab_scores(qs, ws, qbs, row, H, P, cb, sv);
#pragma unroll
        for (int i = 0; i < PT; ++i) cnt[i] += (live && ahead<int>(sv[i], rel, ts[i], trel[i])) ? 1 : 0;   // (false for NaN)
    }

    // lane i adds pair i's count over the wave to its rank -- one atomic instruction per wave
    int mine = 0;
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        int v = cnt[i];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
        if (lane == i) mine = v;
    }
    // (mine > 0 only for a pair below n_p whose target is ranked: the others wait for +inf)
    if (lane < PT && mine > 0)
        atomicAdd(reinterpret_cast<unsigned long long *>(a.out_rank + p0 + lane), (unsigned long long)mine);
}

}  // namespace
}  // namespace r4r

using namespace r4r;

extern "C" size_t r4r_topk_relu_ws_bytes(int64_t n_q, int64_t n_c, int K, int64_t chunk) {
    return lists_ws_bytes(n_q, n_c, K, chunk, RELU_QT);
}

extern "C" int r4r_topk_relu(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                             const float *c_bias, const float *w, int H, int P, const int64_t *excl_off,
                             const int64_t *excl_ids, int K, int64_t chunk, void *ws, size_t ws_bytes, int64_t *out_ids,
                             float *out_scores, void *stream) {
    const ReluHead h = relu_head(q, q_bias, c, n_c, c_stride, c_bias, w, H, P);
    bool work;
    int rc = topk_check("topk_relu", h, n_q, excl_off, excl_ids, K, chunk, out_ids, out_scores, &work);
    if (rc != R4R_OK || !work) return rc;
    ListsPlan p;
    rc = topk_plan("topk_relu", n_q, n_c, K, chunk, RELU_QT, RELU_QT, ws, ws_bytes, out_ids, out_scores, &p);
    if (rc != R4R_OK) return rc;
    ReluScanArgs a;
    a.q = q; a.q_bias = q_bias; a.c = c; a.c_bias = c_bias; a.w = w;
    a.excl_off = excl_off; a.excl_ids = excl_ids;
    a.out_scores = p.scan_scores; a.out_ids = p.scan_ids;
    a.n_q = n_q; a.n_c = n_c; a.c_stride = c_stride; a.chunk = p.chunk; a.parts = p.parts; a.tiles = p.tiles;
    a.H = H; a.P = P; a.K = K;
    hipStream_t st = as_stream(stream);
    const size_t lds = relu_stage_floats(H, P) * 4 + (size_t)RELU_QT * (size_t)K * 8;
    static_assert((size_t)((RELU_MAX_H + RELU_MAX_P) * RELU_QT + RELU_QT + RELU_MAX_H) * 4 + (size_t)RELU_QT * TOPK_MAX_K * 8 <= 65536,
                  "the staged queries and the lists fit the LDS a launch gets without asking for more");
    hipLaunchKernelGGL(relu_scan_kernel, dim3((unsigned)(p.parts * p.tiles)), dim3(64), lds, st, a);
    return topk_finish(p, check_launch("relu_scan_kernel"), n_q, K, out_ids, out_scores, st);
}

extern "C" int r4r_pair_relu(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                             const float *c_bias, const float *w, int H, int P, const int64_t *q_idx, const int64_t *c_idx,
                             int64_t n, float *out, void *stream) {
    const ReluHead h = relu_head(q, q_bias, c, n_c, c_stride, c_bias, w, H, P);
    bool work;
    const int rc = pair_check("pair_relu", h, n_q, q_idx, c_idx, n, out, &work);
    if (rc != R4R_OK || !work) return rc;
    return launch_pairs(h, q_idx, c_idx, n, out, as_stream(stream));
}

extern "C" int r4r_rank_relu(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                             const float *c_bias, const float *w, int H, int P, const int64_t *q_idx, const int64_t *t_idx,
                             int64_t n_p, const int64_t *excl_off, const int64_t *excl_ids, int64_t chunk, int64_t *out_rank,
                             float *out_score, void *stream) {
    const ReluHead h = relu_head(q, q_bias, c, n_c, c_stride, c_bias, w, H, P);
    bool work;
    int rc = rank_check("rank_relu", h, n_q, q_idx, t_idx, n_p, excl_off, excl_ids, chunk, out_rank, out_score, &work);
    if (rc != R4R_OK || !work) return rc;
    ChunkPlan p;
    rc = rank_plan("rank_relu", n_p, n_c, chunk, RELU_QT, RELU_QT, &p);
    if (rc != R4R_OK) return rc;
    ReluRankArgs a;
    a.q = q; a.q_bias = q_bias; a.c = c; a.c_bias = c_bias; a.w = w; a.q_idx = q_idx; a.t_idx = t_idx;
    a.t_score = out_score; a.out_rank = out_rank;
    a.n_p = n_p; a.n_c = n_c; a.c_stride = c_stride; a.chunk = p.chunk; a.tiles = p.tiles; a.H = H; a.P = P;
    hipStream_t st = as_stream(stream);
    rc = launch_rank_targets(h, q_idx, t_idx, n_p, out_score, out_rank, st);
    if (rc != R4R_OK) return rc;
    hipLaunchKernelGGL(rank_relu_scan_kernel, dim3((unsigned)(p.parts * p.tiles)), dim3(64), relu_stage_floats(H, P) * 4, st, a);
    return rank_finish(h, check_launch("rank_relu_scan_kernel"), q_idx, t_idx, n_p, excl_off, excl_ids, out_score, out_rank, st);
}

// Slates (slate_device.h): the K best of, and the place of a target among, per-query candidate lists
extern "C" int r4r_slate_topk_relu(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c,
                                   int64_t c_stride, const float *c_bias, const float *w, int H, int P,
                                   const int64_t *q_idx, const int64_t *slate_off, const int64_t *slate_ids,
                                   int64_t n_s, int64_t max_len, const int64_t *excl_off, const int64_t *excl_ids,
                                   int K, void *ws, size_t ws_bytes, int64_t *out_ids, float *out_scores, void *stream) {
    const ReluHead h = relu_head(q, q_bias, c, n_c, c_stride, c_bias, w, H, P);
    return slate_topk_call("slate_topk_relu", h, n_q, q_idx, slate_off, slate_ids, n_s, max_len, excl_off, excl_ids, K,
                           ws, ws_bytes, out_ids, out_scores, stream);
}

extern "C" int r4r_slate_rank_relu(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c,
                                   int64_t c_stride, const float *c_bias, const float *w, int H, int P,
                                   const int64_t *q_idx, const int64_t *t_idx, const int64_t *slate_off,
                                   const int64_t *slate_ids, int64_t n_p, int64_t max_len, const int64_t *excl_off,
                                   const int64_t *excl_ids, int64_t *out_rank, float *out_score, void *stream) {
    const ReluHead h = relu_head(q, q_bias, c, n_c, c_stride, c_bias, w, H, P);
    return slate_rank_call("slate_rank_relu", h, n_q, q_idx, t_idx, slate_off, slate_ids, n_p, max_len, excl_off,
                           excl_ids, out_rank, out_score, stream);
}

// Catalogue top-K: r4r_topk_dot (include/r4r.h, "Catalogue recommendation").
//
// score(u, i) = (dot(q[u], c[i]) + c_bias[i]) + q_bias[u], dot an ascending fmaf chain from +0 -- computed by
// v_mfma_f32_16x16x4_f32 (bitwise that chain; MFMA t sums j = 4t .. 4t+3 in order, lane l supplies j = 4t + (l >> 4)),
// never written to memory: every score is compared in registers with its query's current K-th best and only the
// survivors (of the order of K ln(chunk / K) per query and chunk) reach the sorted per-query list in LDS.
//
// Launch 1, topk_scan_kernel: one WAVE per workgroup = (query tile of 16 * NQ queries) x (chunk of candidates).  The
// wave keeps its queries' A fragments in registers for the whole chunk, streams 16-candidate slabs (B fragments straight
// from global memory: one dword per lane and MFMA, the four lanes of a candidate row read 16 contiguous bytes; the next
// slab's loads are in flight across this slab's MFMAs) and owns its lists, so the kernel has no barrier.  Consecutive
// workgroups are the query tiles of ONE chunk, so that the tiles of a chunk can share what the first of them fetched (the
// intent; DESIGN.md 4.14 has what the counters show).  Measured there: the dword-granular loads, not HBM or the matrix
// pipe, bound the scan.
// Launch 2, topk_merge_kernel: one workgroup per query merges the chunks' partial lists (skipped for a single chunk:
// launch 1 then writes the result itself).
//
// The order (score descending, id ascending; never -inf, NaN or an excluded id) is total and every score's bits depend
// on its own (u, i) only, so the result does not depend on the chunking, the tile or the other queries of the call.
//
// r4r_rank_dot, at the end of the file: the same stream with counters in place of lists -- the rank of explicit targets.
//
// This file has the two streams, the merge and the head of this form (DotHead: the scalar form of the chain); what sits
// around the streams, the scalar kernels over a head and the host checks and plans are topk_device.h's, shared with
// topk_relu.hip and topk_hmlp.hip.
#include <math.h>

#include "common.h"
#include "slate_device.h"
#include "topk_device.h"

namespace r4r {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TOPK_MAX_D = 256;
constexpr int64_t TOPK_WIDE_TILE_MIN_Q = 512;   // below this 16-query tiles alone fill the machine with fewer, longer chunks

// 16-query sub-tiles per wave: four share every B fragment (the candidate matrix is re-read once per tile); above D = 128 the
// A fragments of four no longer fit the registers
inline int topk_nq(int64_t n_q, int D) { return (n_q >= TOPK_WIDE_TILE_MIN_Q && D <= 128) ? 4 : 1; }

// The tile width the chunk rule (topk_device.h's resolve_chunk) counts with.  Not a function of D (r4r_topk_dot_ws_bytes has
// none): the tiles are counted as topk_nq counts them for D <= 128.  From 512 queries on with D > 128 the scan runs
// 16-query tiles over chunks sized for 64-query ones: four times the intended waves, the same result.
inline int topk_chunk_tile(int64_t n_q) { return 16 * topk_nq(n_q, 0); }

// The head of this form: the scalar form of the chain the matrix pipe computes
struct DotHead {
    const float *q, *q_bias, *c, *c_bias;
    int64_t n_c, c_stride;
    int D;

    __device__ __forceinline__ float q_bias_of(int64_t u) const { return q_bias ? q_bias[u] : 0.f; }
    __device__ __forceinline__ float score(int64_t u, int64_t i, float qb) const {
        float dot = 0.f;
        for (int j = 0; j < D; ++j) dot = __builtin_fmaf(q[u * D + j], c[i * c_stride + j], dot);
        return (dot + (c_bias ? c_bias[i] : 0.f)) + qb;
    }
    __device__ __forceinline__ float score(int64_t u, int64_t i) const { return score(u, i, q_bias_of(u)); }

    static constexpr const char *width_name = "D";
    int width() const { return D; }
    int ranges(const char *fn) const {
        R4R_REQUIRE(D >= 0 && D <= TOPK_MAX_D, "%s: D = %d outside 0 .. %d", fn, D, TOPK_MAX_D);
        return R4R_OK;
    }
    int weights(const char *) const { return R4R_OK; }
};

inline DotHead dot_head(const float *q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                        const float *c_bias, int D) {
    DotHead h;
    h.q = q; h.q_bias = q_bias; h.c = c; h.c_bias = c_bias;
    h.n_c = n_c; h.c_stride = c_stride; h.D = D;
    return h;
}

struct ScanArgs {
    const float *q, *q_bias, *c, *c_bias;
    const int64_t *excl_off, *excl_ids;
    float *out_scores;        // [n_q, parts, K]
    int64_t *out_ids;
    int64_t n_q, n_c, c_stride, chunk, parts, tiles;
    int D, K;
};

// KT: MFMAs per slab (D <= 4 KT), NQ: 16-query sub-tiles per wave, SL: slabs per iteration (loads in flight for small D)
template <int KT, int NQ, int SL>
__global__ __launch_bounds__(64) void topk_scan_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_lds[];
    constexpr int QT = 16 * NQ;
    const int K = a.K, D = a.D;
    float *sc = reinterpret_cast<float *>(topk_lds);          // [QT][K]
    int *id = reinterpret_cast<int *>(sc + QT * K);            // [QT][K]  candidate - chunk begin

    const int lane = threadIdx.x;
    const int row = lane & 15, kq = lane >> 4;
    const ChunkGeom g = chunk_geom(a.tiles, QT, a.chunk, a.n_c);
    const int64_t u0 = g.first, c_begin = g.c_begin, c_end = g.c_end;

    for (int i = lane; i < QT * K; i += 64) { sc[i] = -INFINITY; id[i] = fill_id<int>::value; }

    // A fragments: lane (row, kq) holds q[u0 + 16 s + row][4 t + kq]; zero beyond n_q and beyond D
    float af[NQ][KT];
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
        const int64_t u = u0 + 16 * s + row;
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int j = 4 * t + kq;
            af[s][t] = (u < a.n_q && j < D) ? a.q[u * D + j] : 0.f;
        }
    }
    // the accumulator layout: lane holds candidate `row` against queries 16 s + 4 kq + r
    float qb[NQ][4], thr[NQ][4];
#pragma unroll
    for (int s = 0; s < NQ; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t u = u0 + 16 * s + 4 * kq + r;
            qb[s][r] = (a.q_bias != nullptr && u < a.n_q) ? a.q_bias[u] : 0.f;
            thr[s][r] = (u < a.n_q) ? -INFINITY : INFINITY;          // rows past n_q never survive
        }
    wave_lds_fence();

    // B fragments: lane (row, kq) holds c[slab + row][4 t + kq].  The loads are unconditional and nothing reads their
    // results before `take`, after the current slab's MFMAs and epilogue: the next slab's loads stay in flight across
    // them.  A column past D reads column D - 1 and is zeroed in `take`, a row of the NEXT chunk is read and ignored,
    // a row past the table reads the table's last row.
    int jo[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) jo[t] = (4 * t + kq < D) ? 4 * t + kq : (D > 0 ? D - 1 : 0);
    float bf[SL][KT], bn[SL][KT], cb[SL], cbn[SL];
#pragma unroll
    for (int l = 0; l < SL; ++l) {
        cbn[l] = 0.f;
#pragma unroll
        for (int t = 0; t < KT; ++t) bn[l][t] = 0.f;
    }
    auto load = [&](int64_t base) {
#pragma unroll
        for (int l = 0; l < SL; ++l) {
            const int64_t i = base + 16 * l + row;
            const int64_t ic = i < a.n_c ? i : a.n_c - 1;
            const float *src = a.c + ic * a.c_stride;
            if (D > 0) {
#pragma unroll
                for (int t = 0; t < KT; ++t) bn[l][t] = src[jo[t]];
            }
            if (a.c_bias != nullptr) cbn[l] = a.c_bias[ic];
        }
    };
    auto take = [&]() {
#pragma unroll
        for (int l = 0; l < SL; ++l) {
            cb[l] = cbn[l];
#pragma unroll
            for (int t = 0; t < KT; ++t) bf[l][t] = (4 * t + kq < D) ? bn[l][t] : 0.f;
        }
    };

    constexpr int STEP = 16 * SL;
    if (c_begin < c_end) load(c_begin);
    take();
    for (int64_t base = c_begin; base < c_end; base += STEP) {
        if (base + STEP < c_end) load(base + STEP);
#pragma unroll
        for (int l = 0; l < SL; ++l) {
            f32x4 acc[NQ];
#pragma unroll
            for (int s = 0; s < NQ; ++s) acc[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int s = 0; s < NQ; ++s)
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s][t], bf[l][t], acc[s], 0, 0, 0);
            const int64_t cand = base + 16 * l + row;
            const bool live = cand < c_end;
            bool any = false;
            float sv[NQ][4];
#pragma unroll
            for (int s = 0; s < NQ; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sv[s][r] = (acc[s][r] + cb[l]) + qb[s][r];
                    any |= live && sv[s][r] > thr[s][r];
                }
            if (__ballot(any) == 0) continue;
            // survivors, one at a time (wave-uniform control flow from here on)
#pragma unroll
            for (int s = 0; s < NQ; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    unsigned long long m = __ballot(live && sv[s][r] > thr[s][r]);
                    while (m) {
                        const int src = __builtin_ctzll(m);
                        m &= m - 1;
                        const float v = lane_value(sv[s][r], src);
                        const int ql = 16 * s + 4 * (src >> 4) + r;
                        const int64_t ci = base + 16 * l + (src & 15);
                        if (!(v > lane_value(thr[s][r], src))) continue;         // (an earlier survivor raised the bar)
                        if (is_excluded(a.excl_off, a.excl_ids, u0 + ql, ci)) continue;
                        const float bar = list_insert<int>(sc + ql * K, id + ql * K, K, v, (int)(ci - c_begin), lane);
                        if (kq == (src >> 4)) thr[s][r] = bar;                   // the lanes that hold this query
                    }
                }
        }
        take();
    }

    // the partial lists, filled up with (-inf, -1)
    for (int ql = 0; ql < QT; ++ql) {
        const int64_t u = u0 + ql;
        if (u >= a.n_q) break;
        const int64_t o = (u * a.parts + g.part) * K;
        for (int p = lane; p < K; p += 64) {
            const int ci = id[ql * K + p];
            a.out_scores[o + p] = sc[ql * K + p];                                 // (-inf in an unused slot)
            a.out_ids[o + p] = ci != fill_id<int>::value ? c_begin + ci : (int64_t)-1;
        }
    }
}

// One workgroup per query: every wave merges a share of the parts * K partial entries into a list of its own, then
// wave 0 merges the other waves' lists into its list and writes the result.
__global__ __launch_bounds__(MERGE_THREADS) void topk_merge_kernel(const float *__restrict__ ps, const int64_t *__restrict__ pi,
                                                                    int64_t parts, int K, int64_t *__restrict__ out_ids,
                                                                    float *__restrict__ out_scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_lds[];
    constexpr int NW = MERGE_THREADS / 64;
    int64_t *id = reinterpret_cast<int64_t *>(topk_lds);       // [NW][K]
    float *sc = reinterpret_cast<float *>(id + NW * K);        // [NW][K]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t u = blockIdx.x;
    const int64_t total = parts * K;
    ps += u * total;
    pi += u * total;
    float *msc = sc + w * K;
    int64_t *mid = id + w * K;
    for (int p = lane; p < K; p += 64) { msc[p] = -INFINITY; mid[p] = fill_id<int64_t>::value; }
    wave_lds_fence();
    float bar = -INFINITY;                                     // this wave's K-th best (wave-uniform)
    auto offer = [&](bool want, float s, int64_t i) {
        unsigned long long m = __ballot(want);
        while (m) {
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const float v = lane_value(s, src);
            const int64_t ci = __shfl(i, src);
            if (v >= bar) bar = list_insert<int64_t>(msc, mid, K, v, ci, lane);
        }
    };
    constexpr int UN = 4;
    for (int64_t e0 = (int64_t)w * 64 * UN; e0 < total; e0 += (int64_t)MERGE_THREADS * UN) {
        float s[UN];
        int64_t i[UN];
#pragma unroll
        for (int k = 0; k < UN; ++k) {
            const int64_t e = e0 + 64 * k + lane;
            i[k] = e < total ? pi[e] : -1;
            s[k] = e < total ? ps[e] : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < UN; ++k) offer(i[k] >= 0 && s[k] >= bar, s[k], i[k]);
    }
    __syncthreads();
    if (w == 0) {
        for (int o = 1; o < NW; ++o)
            for (int p0 = 0; p0 < K; p0 += 64) {
                const int p = p0 + lane;
                const float s = p < K ? sc[o * K + p] : -INFINITY;
                const int64_t i = p < K ? id[o * K + p] : fill_id<int64_t>::value;
                offer(i != fill_id<int64_t>::value && s >= bar, s, i);
            }
        for (int p = lane; p < K; p += 64) {
            out_scores[u * K + p] = sc[p];
            out_ids[u * K + p] = id[p] != fill_id<int64_t>::value ? id[p] : (int64_t)-1;
        }
    }
}

template <int KT, int NQ, int SL>
int launch_scan(const ScanArgs &a, hipStream_t st) {
    const size_t lds = (size_t)16 * NQ * (size_t)a.K * 8;
    static_assert((size_t)16 * NQ * TOPK_MAX_K * 8 <= 65536, "the lists fit the LDS a launch gets without asking for more");
    hipLaunchKernelGGL((topk_scan_kernel<KT, NQ, SL>), dim3((unsigned)(a.parts * a.tiles)), dim3(64), lds, st, a);
    return check_launch("topk_scan_kernel");
}

template <int NQ>
int launch_scan_d(const ScanArgs &a, hipStream_t st) {
    // (slabs per iteration: a lone 16-query tile is bound by the stream and keeps more loads in flight)
    if (a.D <= 8) return launch_scan<2, NQ, 4>(a, st);
    if (a.D <= 16) return launch_scan<4, NQ, 4>(a, st);
    if (a.D <= 32) return launch_scan<8, NQ, NQ == 1 ? 4 : 2>(a, st);
    if (a.D <= 64) return launch_scan<16, NQ, NQ == 1 ? 2 : 1>(a, st);
    if constexpr (NQ == 1) {                                    // (topk_nq: wider tiles stop at D = 128)
        if (a.D > 128) return launch_scan<64, 1, 1>(a, st);
    }
    return launch_scan<32, NQ, 1>(a, st);
}

}  // namespace

int topk_launch_merge(const float *ps, const int64_t *pi, int64_t n_q, int64_t parts, int K, int64_t *out_ids,
                      float *out_scores, hipStream_t st) {
    const size_t lds = (size_t)(MERGE_THREADS / 64) * (size_t)K * 12;
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)n_q), dim3(MERGE_THREADS), lds, st, ps, pi, parts, K, out_ids,
                       out_scores);
    return check_launch("topk_merge_kernel");
}

}  // namespace r4r

using namespace r4r;

extern "C" size_t r4r_topk_dot_ws_bytes(int64_t n_q, int64_t n_c, int K, int64_t chunk) {
    return lists_ws_bytes(n_q, n_c, K, chunk, topk_chunk_tile(n_q));
}

extern "C" int r4r_topk_dot(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                            const float *c_bias, int D, const int64_t *excl_off, const int64_t *excl_ids, int K,
                            int64_t chunk, void *ws, size_t ws_bytes, int64_t *out_ids, float *out_scores, void *stream) {
    const DotHead h = dot_head(q, q_bias, c, n_c, c_stride, c_bias, D);
    bool work;
    int rc = topk_check("topk_dot", h, n_q, excl_off, excl_ids, K, chunk, out_ids, out_scores, &work);
    if (rc != R4R_OK || !work) return rc;
    const int NQ = topk_nq(n_q, D);
    ListsPlan p;
    rc = topk_plan("topk_dot", n_q, n_c, K, chunk, topk_chunk_tile(n_q), 16 * NQ, ws, ws_bytes, out_ids, out_scores, &p);
    if (rc != R4R_OK) return rc;
    ScanArgs a;
    a.q = q; a.q_bias = q_bias; a.c = c; a.c_bias = c_bias;
    a.excl_off = excl_off; a.excl_ids = excl_ids;
    a.out_scores = p.scan_scores; a.out_ids = p.scan_ids;
    a.n_q = n_q; a.n_c = n_c; a.c_stride = c_stride; a.chunk = p.chunk; a.parts = p.parts; a.tiles = p.tiles;
    a.D = D; a.K = K;
    hipStream_t st = as_stream(stream);
    rc = NQ == 4 ? launch_scan_d<4>(a, st) : launch_scan_d<1>(a, st);
    return topk_finish(p, rc, n_q, K, out_ids, out_scores, st);
}

extern "C" int r4r_pair_dot(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                            const float *c_bias, int D, const int64_t *q_idx, const int64_t *c_idx, int64_t n, float *out,
                            void *stream) {
    const DotHead h = dot_head(q, q_bias, c, n_c, c_stride, c_bias, D);
    bool work;
    const int rc = pair_check("pair_dot", h, n_q, q_idx, c_idx, n, out, &work);
    if (rc != R4R_OK || !work) return rc;
    return launch_pairs(h, q_idx, c_idx, n, out, as_stream(stream));
}

// ---------------------------------------------------------------------------------------------------------------------
// r4r_rank_dot: the rank of explicit targets.  Pair p = (query row q_idx[p], target t_idx[p]); its rank is the number of
// candidates ahead of the target in the order above -- a count, so the scan's lists, survivors and merge fall away.
//   A  rank_target_kernel<DotHead>   one thread per pair: the scalar chain -> out_score[p]; out_rank[p] = 0, or -1 for
//                                    a target whose own score is -inf or NaN (never touched again)
//   B  rank_scan_kernel              the scan's stream over a tile of 16 * NQ PAIRS (A fragments gathered through q_idx)
//                                    and a chunk of candidates; the epilogue compares every sum with the pair's target
//                                    in registers and counts; one 64-bit integer atomic per (pair, chunk)
//   C  rank_excl_kernel<DotHead>     only with exclusions: B counted the excluded ids too; one wave per pair recomputes
//                                    the scalar chain of its query row's excluded ids and subtracts those that were
//                                    ahead.  Exact, because a score's bits depend on its own pair only (MFMA chain ==
//                                    scalar chain).
// (A and C: topk_device.h.)
// Integer atomics only: the result depends on no order, no chunking, no tiling and no grouping of the pairs.
namespace r4r {
namespace {

#ifndef RANK_WIDE_TILE_MIN_P
#define RANK_WIDE_TILE_MIN_P TOPK_WIDE_TILE_MIN_Q      // (the scan's threshold; DESIGN.md 4.15 has the A/B that argues for less)
#endif

struct RankArgs {
    const float *q, *q_bias, *c, *c_bias;
    const int64_t *q_idx, *t_idx;
    const float *t_score;     // out_score, written by launch A
    int64_t *out_rank;
    int64_t n_p, n_c, c_stride, chunk, tiles;
    int D;
};

// KT, NQ, SL as in topk_scan_kernel; the streaming loop is that kernel's, kept apart from it on purpose
template <int KT, int NQ, int SL>
__global__ __launch_bounds__(64) void rank_scan_kernel(RankArgs a) {
    constexpr int PT = 16 * NQ;
    const int D = a.D;
    const int lane = threadIdx.x;
    const int row = lane & 15, kq = lane >> 4;
    // (chunk_geom, written out: through the helper this kernel's registers are allocated differently from end to end)
    const int64_t tile = blockIdx.x % a.tiles, part = blockIdx.x / a.tiles;
    const int64_t p0 = tile * PT;
    const int64_t c_begin = part * a.chunk;
    const int64_t c_end = (c_begin + a.chunk < a.n_c) ? c_begin + a.chunk : a.n_c;
    const int c_len = (int)(c_end - c_begin);                  // (chunk <= 2^30)

    // Everything the wave keeps for the chunk is loaded UNCONDITIONALLY from clamped addresses and selected afterwards (a
    // pair past n_p reads pair n_p - 1, a column past D reads column D - 1): a guard per load makes hipcc branch around
    // each and wait for every dependent chain in turn, which costs a short chunk more than its stream.
    const int64_t p_last = a.n_p - 1;
    int jo[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) jo[t] = (4 * t + kq < D) ? 4 * t + kq : (D > 0 ? D - 1 : 0);
    // A fragments: lane (row, kq) holds q[q_idx[p0 + 16 s + row]][4 t + kq]; zero beyond n_p and beyond D
    float af[NQ][KT];
#pragma unroll
    for (int s = 0; s < NQ; ++s) {
        const int64_t p = p0 + 16 * s + row;
        const float *src = a.q + a.q_idx[p < a.n_p ? p : p_last] * D;
#pragma unroll
        for (int t = 0; t < KT; ++t) af[s][t] = 0.f;
        if (D > 0) {
#pragma unroll
            for (int t = 0; t < KT; ++t) af[s][t] = src[jo[t]];
        }
#pragma unroll
        for (int t = 0; t < KT; ++t) af[s][t] = (p < a.n_p && 4 * t + kq < D) ? af[s][t] : 0.f;
    }
    // the accumulator layout: lane holds candidate `row` against pairs 16 s + 4 kq + r.  Of each pair: its query bias, its
    // target's score and its target's id relative to the chunk (-1: before it, so no tie is ahead; INT_MAX: behind it, so
    // every tie is).  A pair past n_p or at -1 waits for a score above +inf with an id below -1: it counts nothing.
    float qb[NQ][4], ts[NQ][4];
    int trel[NQ][4], cnt[NQ][4];
#pragma unroll
    for (int s = 0; s < NQ; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t p = p0 + 16 * s + 4 * kq + r;
            const int64_t pc = p < a.n_p ? p : p_last;
            const float st = a.t_score[pc];
            const int64_t d = a.t_idx[pc] - c_begin;
            qb[s][r] = a.q_bias != nullptr ? a.q_bias[a.q_idx[pc]] : 0.f;
            const bool ranked = p < a.n_p && st > -INFINITY;   // (false for NaN)
            ts[s][r] = ranked ? st : INFINITY;
            trel[s][r] = !ranked || d < 0 ? -1 : (d > 0x7fffffff ? 0x7fffffff : (int)d);
            cnt[s][r] = 0;
        }

    // B fragments: lane (row, kq) holds c[slab + row][4 t + kq].  The loads are unconditional and nothing reads their
    // results before `take`, after the current slab's MFMAs and epilogue.  A column past D reads column D - 1 and is
    // zeroed in `take`, a row of the NEXT chunk is read and ignored, a row past the table reads the table's last row.
    float bf[SL][KT], bn[SL][KT], cb[SL], cbn[SL];
#pragma unroll
    for (int l = 0; l < SL; ++l) {
        cbn[l] = 0.f;
#pragma unroll
        for (int t = 0; t < KT; ++t) bn[l][t] = 0.f;
    }
    auto load = [&](int64_t base) {
#pragma unroll
        for (int l = 0; l < SL; ++l) {
            const int64_t i = base + 16 * l + row;
            const int64_t ic = i < a.n_c ? i : a.n_c - 1;
            const float *src = a.c + ic * a.c_stride;
            if (D > 0) {
#pragma unroll
                for (int t = 0; t < KT; ++t) bn[l][t] = src[jo[t]];
            }
            if (a.c_bias != nullptr) cbn[l] = a.c_bias[ic];
        }
    };
    auto take = [&]() {
#pragma unroll
        for (int l = 0; l < SL; ++l) {
            cb[l] = cbn[l];
#pragma unroll
            for (int t = 0; t < KT; ++t) bf[l][t] = (4 * t + kq < D) ? bn[l][t] : 0.f;
        }
    };

    constexpr int STEP = 16 * SL;
    if (c_begin < c_end) load(c_begin);
    take();
    for (int64_t base = c_begin; base < c_end; base += STEP) {
        if (base + STEP < c_end) load(base + STEP);
#pragma unroll
        for (int l = 0; l < SL; ++l) {
            f32x4 acc[NQ];
#pragma unroll
            for (int s = 0; s < NQ; ++s) acc[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int s = 0; s < NQ; ++s)
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s][t], bf[l][t], acc[s], 0, 0, 0);
            const int rel = (int)(base - c_begin) + 16 * l + row;
            const bool live = rel < c_len;
#pragma unroll
            for (int s = 0; s < NQ; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sv = (acc[s][r] + cb[l]) + qb[s][r];
                    cnt[s][r] += (live && ahead<int>(sv, rel, ts[s][r], trel[s][r])) ? 1 : 0;       // (false for a NaN sum)
                }
        }
        take();
    }

    // the 16 lanes of one kq hold one pair's counters: sum over the low four lane bits, then lane row = 4 s + r adds pair
    // 16 s + 4 kq + r's count to its rank -- one atomic instruction per wave
    int mine = 0;
#pragma unroll
    for (int s = 0; s < NQ; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            int v = cnt[s][r];
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
            if (row == 4 * s + r) mine = v;
        }
    if (row < 4 * NQ && mine > 0) {
        const int64_t p = p0 + 16 * (row >> 2) + 4 * kq + (row & 3);
        // (mine > 0 only for a pair below n_p whose target is ranked: the others wait for +inf)
        atomicAdd(reinterpret_cast<unsigned long long *>(a.out_rank + p), (unsigned long long)mine);
    }
}

inline int rank_nq(int64_t n_p, int D) { return (n_p >= RANK_WIDE_TILE_MIN_P && D <= 128) ? 4 : 1; }

template <int KT, int NQ, int SL>
int launch_rank(const RankArgs &a, int64_t parts, hipStream_t st) {
    hipLaunchKernelGGL((rank_scan_kernel<KT, NQ, SL>), dim3((unsigned)(parts * a.tiles)), dim3(64), 0, st, a);
    return check_launch("rank_scan_kernel");
}

template <int NQ>
int launch_rank_d(const RankArgs &a, int64_t parts, hipStream_t st) {
    // (KT and SL by D and NQ exactly as launch_scan_d picks them)
    if (a.D <= 8) return launch_rank<2, NQ, 4>(a, parts, st);
    if (a.D <= 16) return launch_rank<4, NQ, 4>(a, parts, st);
    if (a.D <= 32) return launch_rank<8, NQ, NQ == 1 ? 4 : 2>(a, parts, st);
    if (a.D <= 64) return launch_rank<16, NQ, NQ == 1 ? 2 : 1>(a, parts, st);
    if constexpr (NQ == 1) {
        if (a.D > 128) return launch_rank<64, 1, 1>(a, parts, st);
    }
    return launch_rank<32, NQ, 1>(a, parts, st);
}

}  // namespace
}  // namespace r4r

extern "C" int r4r_rank_dot(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                            const float *c_bias, int D, const int64_t *q_idx, const int64_t *t_idx, int64_t n_p,
                            const int64_t *excl_off, const int64_t *excl_ids, int64_t chunk, int64_t *out_rank,
                            float *out_score, void *stream) {
    const DotHead h = dot_head(q, q_bias, c, n_c, c_stride, c_bias, D);
    bool work;
    int rc = rank_check("rank_dot", h, n_q, q_idx, t_idx, n_p, excl_off, excl_ids, chunk, out_rank, out_score, &work);
    if (rc != R4R_OK || !work) return rc;
    const int NQ = rank_nq(n_p, D);
    ChunkPlan p;
    rc = rank_plan("rank_dot", n_p, n_c, chunk, topk_chunk_tile(n_p), 16 * NQ, &p);
    if (rc != R4R_OK) return rc;
    RankArgs a;
    a.q = q; a.q_bias = q_bias; a.c = c; a.c_bias = c_bias; a.q_idx = q_idx; a.t_idx = t_idx;
    a.t_score = out_score; a.out_rank = out_rank;
    a.n_p = n_p; a.n_c = n_c; a.c_stride = c_stride; a.chunk = p.chunk; a.tiles = p.tiles; a.D = D;
    hipStream_t st = as_stream(stream);
    rc = launch_rank_targets(h, q_idx, t_idx, n_p, out_score, out_rank, st);
    if (rc != R4R_OK) return rc;
    rc = NQ == 4 ? launch_rank_d<4>(a, p.parts, st) : launch_rank_d<1>(a, p.parts, st);
    return rank_finish(h, rc, q_idx, t_idx, n_p, excl_off, excl_ids, out_score, out_rank, st);
}

// Slates (slate_device.h): the K best of, and the place of a target among, per-query candidate lists
extern "C" int r4r_slate_topk_dot(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c,
                                  int64_t c_stride, const float *c_bias, int D, const int64_t *q_idx,
                                  const int64_t *slate_off, const int64_t *slate_ids, int64_t n_s, int64_t max_len,
                                  const int64_t *excl_off, const int64_t *excl_ids, int K, void *ws, size_t ws_bytes,
                                  int64_t *out_ids, float *out_scores, void *stream) {
    const DotHead h = dot_head(q, q_bias, c, n_c, c_stride, c_bias, D);
    return slate_topk_call("slate_topk_dot", h, n_q, q_idx, slate_off, slate_ids, n_s, max_len, excl_off, excl_ids, K,
                           ws, ws_bytes, out_ids, out_scores, stream);
}

extern "C" int r4r_slate_rank_dot(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c,
                                  int64_t c_stride, const float *c_bias, int D, const int64_t *q_idx,
                                  const int64_t *t_idx, const int64_t *slate_off, const int64_t *slate_ids, int64_t n_p,
                                  int64_t max_len, const int64_t *excl_off, const int64_t *excl_ids, int64_t *out_rank,
                                  float *out_score, void *stream) {
    const DotHead h = dot_head(q, q_bias, c, n_c, c_stride, c_bias, D);
    return slate_rank_call("slate_rank_dot", h, n_q, q_idx, t_idx, slate_off, slate_ids, n_p, max_len, excl_off,
                           excl_ids, out_rank, out_score, stream);
}

extern "C" int r4r_slate_piece(void) { return SLATE_PIECE; }

extern "C" size_t r4r_slate_ws_bytes(int64_t n_s, int64_t max_len, int K) { return slate_lists_ws_bytes(n_s, max_len, K); }

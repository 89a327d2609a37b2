// Slates (include/r4r.h, "Slates"): the K best of, and the place of a target among, a per-query candidate LIST instead
// of the whole catalogue -- r4r_slate_topk_<form> / r4r_slate_rank_<form>.  Written once over a score head
// (topk_device.h) and instantiated in each form's file: the scalar chain h.score(u, i, qb) is bitwise what the form's
// scan computes, so a slate that is the whole catalogue gives the scan's lists and ranks.
//   device  slate_lists_kernel<Head>, slate_rank_kernel<Head>
//   host    the piece rule, the workspace size, the argument checks and the sequence of the two calls
// A work item is (slate, piece): SLATE_PIECE consecutive entries of the slate; the LAST piece of a slate takes whatever
// is left, so an understated max_len costs time and no entry.  One wave per work item, SLATE_WAVES of them per
// workgroup as rank_excl_kernel lays them out; no barrier.
//
// SLATE_PIECE = 256.  A place is a count: the piece's (score, id) are staged in LDS and every lane
// counts, for each of its SLATE_PIECE / 64 = 4 entries, the staged entries ahead of it -- one broadcast read per staged
// entry and four compares, so a piece costs PIECE reads and PIECE^2 / 64 compares per lane.  At 256 that is 256 LDS round
// trips, of the order of one hmlp chain at L = 64; at 1,024 it would be sixteen times the compares for a quarter of the
// partial lists, and the merge of four lists of K <= 128 is the cheaper side.  256 also keeps the stage at 3 KiB per
// wave (18 KiB per workgroup with the lists), so LDS never bounds the occupancy, and a slate of 100 -- the sampled-
// negative protocol -- is a single piece without a merge.
#pragma once
#include <math.h>

#include "common.h"
#include "topk_device.h"

namespace r4r {

constexpr int SLATE_PIECE = 256;
constexpr int SLATE_WAVES = 4;
constexpr int SLATE_OWN = SLATE_PIECE / 64;    // staged entries per lane

struct SlateListArgs {
    const int64_t *q_idx, *off, *ids, *excl_off, *excl_ids;
    float *out_scores;        // [n_s, parts, K]
    int64_t *out_ids;
    int64_t n_s, parts;
    int K;
};

struct SlateRankArgs {
    const int64_t *q_idx, *t_idx, *off, *ids, *excl_off, *excl_ids;
    const float *t_score;     // out_score, written by rank_target_kernel
    int64_t *out_rank;
    int64_t n_p, parts;
};

// the entries [begin, end) of slate_ids that piece j of `parts` covers in the slate [lo, hi)
__device__ __forceinline__ void slate_piece(int64_t lo, int64_t hi, int64_t j, int64_t parts, int64_t *begin, int64_t *end) {
    int64_t b = lo + j * SLATE_PIECE;
    if (b > hi) b = hi;
    *begin = b;
    *end = (j == parts - 1 || b + SLATE_PIECE > hi) ? hi : b + SLATE_PIECE;
}

// The K best of one piece -> the partial list (slate, piece).  Entries outside [0, n_c), excluded for the slate's query
// row or scored -inf / NaN are staged as (-inf, fill_id): never ahead of a real entry, never stored.  The first round of
// a piece stores every entry whose place is below K AT its place; a last piece longer than SLATE_PIECE (max_len
// understated) takes further rounds, whose survivors go through list_insert.
template <class Head>
__global__ __launch_bounds__(64 * SLATE_WAVES) void slate_lists_kernel(Head h, SlateListArgs a) {
    __shared__ int64_t stage_id[SLATE_WAVES][SLATE_PIECE];
    __shared__ int64_t list_id[SLATE_WAVES][TOPK_MAX_K];
    __shared__ float stage_sc[SLATE_WAVES][SLATE_PIECE];
    __shared__ float list_sc[SLATE_WAVES][TOPK_MAX_K];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t item = (int64_t)blockIdx.x * SLATE_WAVES + wv;
    if (item >= a.n_s * a.parts) return;                       // (wave-uniform; the kernel has no barrier)
    const int64_t s = item / a.parts, j = item - s * a.parts;
    const int K = a.K;
    float *ssc = stage_sc[wv], *lsc = list_sc[wv];
    int64_t *sid = stage_id[wv], *lid = list_id[wv];
    int64_t begin, end;
    slate_piece(a.off[s], a.off[s + 1], j, a.parts, &begin, &end);
    const int64_t u = a.q_idx[s];
    const float qb = h.q_bias_of(u);

    for (int p = lane; p < K; p += 64) { lsc[p] = -INFINITY; lid[p] = fill_id<int64_t>::value; }
    wave_lds_fence();
    float bar = -INFINITY;                                     // the list's K-th best after the first round (wave-uniform)
    for (int64_t r0 = begin; r0 < end; r0 += SLATE_PIECE) {
        float ms[SLATE_OWN];
        int64_t mi[SLATE_OWN];
#pragma unroll
        for (int k = 0; k < SLATE_OWN; ++k) {
            const int64_t e = r0 + 64 * k + lane;
            float sv = -INFINITY;
            int64_t ci = fill_id<int64_t>::value;
            if (e < end) {
                const int64_t i = a.ids[e];
                if (i >= 0 && i < h.n_c && !is_excluded(a.excl_off, a.excl_ids, u, i)) {
                    const float v = h.score(u, i, qb);
                    if (v > -INFINITY) { sv = v; ci = i; }     // (false for NaN)
                }
            }
            ms[k] = sv;
            mi[k] = ci;
            ssc[64 * k + lane] = sv;
            sid[64 * k + lane] = ci;
        }
        wave_lds_fence();
        const int n = end - r0 < SLATE_PIECE ? (int)(end - r0) : SLATE_PIECE;
        int place[SLATE_OWN];
#pragma unroll
        for (int k = 0; k < SLATE_OWN; ++k) place[k] = 0;
#pragma unroll 4
        for (int f = 0; f < n; ++f) {
            const float fs = ssc[f];
            const int64_t fi = sid[f];
#pragma unroll
            for (int k = 0; k < SLATE_OWN; ++k) place[k] += ahead<int64_t>(fs, fi, ms[k], mi[k]) ? 1 : 0;
        }
        if (r0 == begin) {
#pragma unroll
            for (int k = 0; k < SLATE_OWN; ++k)
                if (mi[k] != fill_id<int64_t>::value && place[k] < K) { lsc[place[k]] = ms[k]; lid[place[k]] = mi[k]; }
            wave_lds_fence();
            bar = lsc[K - 1];
        } else {
#pragma unroll
            for (int k = 0; k < SLATE_OWN; ++k) {
                unsigned long long m = __ballot(mi[k] != fill_id<int64_t>::value && place[k] < K && ms[k] >= bar);
                while (m) {
                    const int src = __builtin_ctzll(m);
                    m &= m - 1;
                    const float v = lane_value(ms[k], src);
                    const int64_t ci = __shfl(mi[k], src);
                    if (v >= bar) bar = list_insert<int64_t>(lsc, lid, K, v, ci, lane);
                }
            }
        }
        wave_lds_fence();                                      // the next round stages over what this one read
    }

    // the partial list, filled up with (-inf, -1)
    const int64_t o = item * K;
    for (int p = lane; p < K; p += 64) {
        a.out_scores[o + p] = lsc[p];
        a.out_ids[o + p] = lid[p] != fill_id<int64_t>::value ? lid[p] : (int64_t)-1;
    }
}

// After rank_target_kernel<Head> (out_score, out_rank = 0 or -1): a wave counts the entries of its piece that are not
// the target and are AHEAD of it -- a -inf or NaN score never is -- and adds the count to the pair's rank: one 64-bit
// integer atomic per (pair, piece) with a non-zero count.  Exclusions are tested per entry: nothing to correct later.
template <class Head>
__global__ __launch_bounds__(64 * SLATE_WAVES) void slate_rank_kernel(Head h, SlateRankArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * SLATE_WAVES + (threadIdx.x >> 6);
    if (item >= a.n_p * a.parts) return;
    const int64_t p = item / a.parts, j = item - p * a.parts;
    const float st = a.t_score[p];
    if (!(st > -INFINITY)) return;                            // a pair at -1 keeps its -1
    const int64_t u = a.q_idx[p], t = a.t_idx[p];
    int64_t begin, end;
    slate_piece(a.off[p], a.off[p + 1], j, a.parts, &begin, &end);
    const float qb = h.q_bias_of(u);
    int n = 0;
    for (int64_t e0 = begin; e0 < end; e0 += 64) {
        const int64_t e = e0 + lane;
        if (e >= end) continue;
        const int64_t i = a.ids[e];
        if (i < 0 || i >= h.n_c || i == t) continue;
        if (is_excluded(a.excl_off, a.excl_ids, u, i)) continue;
        n += ahead<int64_t>(h.score(u, i, qb), i, st, t) ? 1 : 0;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) n += __shfl_xor(n, m);
    if (lane == 0 && n > 0)
        atomicAdd(reinterpret_cast<unsigned long long *>(a.out_rank + p), (unsigned long long)n);
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side

// pieces per slate of a call: uniform, from the caller's bound on a slate's length
inline int64_t slate_parts(int64_t max_len) {
    const int64_t parts = cdiv(max_len, SLATE_PIECE);
    return parts < 1 ? 1 : parts;
}

// r4r_slate_ws_bytes: the partial lists [n_s, parts, K] of (score, id); nothing for a single piece
inline size_t slate_lists_ws_bytes(int64_t n_s, int64_t max_len, int K) {
    if (n_s <= 0 || max_len <= 0 || K < 1 || K > TOPK_MAX_K) return 0;
    const int64_t parts = slate_parts(max_len);
    if (parts <= 1) return 0;
    return (size_t)n_s * (size_t)parts * (size_t)K * (sizeof(float) + sizeof(int64_t));
}

// What both slate calls refuse in fn's name (n: slates or pairs).  *work = false: nothing to do.
template <class Head>
int slate_check(const char *fn, const Head &h, int64_t n_q, const int64_t *q_idx, const int64_t *slate_off,
                const int64_t *slate_ids, int64_t n, int64_t max_len, const int64_t *excl_off, const int64_t *excl_ids,
                const void *out_a, const void *out_b, bool *work) {
    *work = false;
    if (const int rc = h.ranges(fn)) return rc;
    R4R_REQUIRE(n >= 0 && max_len >= 0 && n_q >= 0 && h.n_c >= 0, "%s: negative size (slates or pairs, max_len, n_q or n_c)", fn);
    R4R_REQUIRE((excl_off == nullptr) == (excl_ids == nullptr), "%s: excl_off and excl_ids go together (both or neither)", fn);
    R4R_REQUIRE(h.c_stride >= h.width(), "%s: c_stride = %lld below %s = %d", fn, (long long)h.c_stride, Head::width_name,
                h.width());
    if (n == 0) return R4R_OK;
    R4R_REQUIRE(out_a != nullptr && out_b != nullptr, "%s: null output", fn);
    if (h.n_c == 0) return R4R_OK;
    R4R_REQUIRE(n_q > 0, "%s: slates into an empty query table", fn);
    if (const int rc = h.weights(fn)) return rc;
    R4R_REQUIRE(q_idx != nullptr && slate_off != nullptr && slate_ids != nullptr && head_rows(h),
                "%s: null pointer (q_idx, slate_off, slate_ids, or q / c with %s > 0)", fn, Head::width_name);
    const int64_t parts = slate_parts(max_len);
    R4R_REQUIRE(n < ((int64_t)1 << 31) && parts < ((int64_t)1 << 31) && cdiv(n * parts, SLATE_WAVES) < ((int64_t)1 << 31),
                "%s: %lld slates x %lld pieces exceed the grid", fn, (long long)n, (long long)parts);
    *work = true;
    return R4R_OK;
}

// r4r_slate_topk_<form>
template <class Head>
int slate_topk_call(const char *fn, const Head &h, int64_t n_q, const int64_t *q_idx, const int64_t *slate_off,
                    const int64_t *slate_ids, int64_t n_s, int64_t max_len, const int64_t *excl_off,
                    const int64_t *excl_ids, int K, void *ws, size_t ws_bytes, int64_t *out_ids, float *out_scores,
                    void *stream) {
    R4R_REQUIRE(K >= 1 && K <= TOPK_MAX_K, "%s: K = %d outside 1 .. %d", fn, K, TOPK_MAX_K);
    bool work;
    int rc = slate_check(fn, h, n_q, q_idx, slate_off, slate_ids, n_s, max_len, excl_off, excl_ids, out_ids, out_scores, &work);
    if (rc != R4R_OK || !work) return rc;
    const size_t need = slate_lists_ws_bytes(n_s, max_len, K);
    if (need > 0 && (ws == nullptr || ws_bytes < need)) {
        set_error("%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
        return R4R_ERR_WORKSPACE;
    }
    SlateListArgs a;
    a.q_idx = q_idx; a.off = slate_off; a.ids = slate_ids; a.excl_off = excl_off; a.excl_ids = excl_ids;
    a.n_s = n_s; a.parts = slate_parts(max_len); a.K = K;
    if (a.parts == 1) {
        a.out_ids = out_ids;
        a.out_scores = out_scores;
    } else {
        a.out_ids = reinterpret_cast<int64_t *>(ws);
        a.out_scores = reinterpret_cast<float *>(a.out_ids + (size_t)n_s * a.parts * K);
    }
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(slate_lists_kernel<Head>, dim3((unsigned)cdiv(n_s * a.parts, SLATE_WAVES)), dim3(64 * SLATE_WAVES), 0,
                       st, h, a);
    rc = check_launch("slate_lists_kernel");
    if (rc != R4R_OK || a.parts == 1) return rc;
    return topk_launch_merge(a.out_scores, a.out_ids, n_s, a.parts, K, out_ids, out_scores, st);
}

// r4r_slate_rank_<form>
template <class Head>
int slate_rank_call(const char *fn, const Head &h, int64_t n_q, const int64_t *q_idx, const int64_t *t_idx,
                    const int64_t *slate_off, const int64_t *slate_ids, int64_t n_p, int64_t max_len,
                    const int64_t *excl_off, const int64_t *excl_ids, int64_t *out_rank, float *out_score, void *stream) {
    bool work;
    int rc = slate_check(fn, h, n_q, q_idx, slate_off, slate_ids, n_p, max_len, excl_off, excl_ids, out_rank, out_score, &work);
    if (rc != R4R_OK || !work) return rc;
    R4R_REQUIRE(t_idx != nullptr, "%s: null pointer (t_idx)", fn);
    SlateRankArgs a;
    a.q_idx = q_idx; a.t_idx = t_idx; a.off = slate_off; a.ids = slate_ids; a.excl_off = excl_off; a.excl_ids = excl_ids;
    a.t_score = out_score; a.out_rank = out_rank;
    a.n_p = n_p; a.parts = slate_parts(max_len);
    hipStream_t st = as_stream(stream);
    rc = launch_rank_targets(h, q_idx, t_idx, n_p, out_score, out_rank, st);
    if (rc != R4R_OK) return rc;
    hipLaunchKernelGGL(slate_rank_kernel<Head>, dim3((unsigned)cdiv(n_p * a.parts, SLATE_WAVES)), dim3(64 * SLATE_WAVES), 0,
                       st, h, a);
    return check_launch("slate_rank_kernel");
}

}  // namespace r4r

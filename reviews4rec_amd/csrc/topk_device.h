// What the catalogue scans share (topk.hip: r4r_*_dot, topk_relu.hip: r4r_*_relu, topk_hmlp.hip: r4r_*_hmlp; * = topk,
// pair, rank): everything but the candidate streams and the score chain of a form.
//   device  the result order, the sorted per-query list of one wave, the chunk geometry of a workgroup, the exclusion
//           search; the three scalar kernels (pairs, rank targets, the exclusion correction) over a score HEAD
//   host    the chunk rule, the workspace size, the argument checks of the three call kinds, the plan of a call, the
//           merge of the chunks' partial lists, the launches of the scalar kernels
// The streaming kernels are each file's own, but for topk_hmlp.hip's and topk_rfm.hip's, which are one text in
// topk_mfma_device.h.  They call chunk_geom and is_excluded, which leave their instructions as they
// were (profiles/topk_shared_isa.txt); clearing and writing back the lists, what a ranked pair waits for and the wave
// sum of its counters did not, and stay written out in each kernel.
// slate_device.h builds on this file: lists and ranks among per-query candidate lists (r4r_slate_topk_<form>,
// r4r_slate_rank_<form>), two more scalar kernels over a head with their own checks and call sequence.
//
// A score head is a trivially copyable struct, passed to kernels by value:
//   q, c, n_c, c_stride             the two tables (rows of width() columns)
//   q_bias_of(u), score(u, i, qb)   device: the scalar chain of one pair -- bitwise what the form's scan computes, so a
//                                   score's bits depend on its own pair only
//   ranges(fn), weights(fn)         host: refuse widths outside the form's limits / missing head weights in fn's name
//   width(), width_name             host: the columns c_stride must cover, and what the messages call them
// (Nothing here is guarded by __HIP_DEVICE_COMPILE__: the device pass instantiates a kernel template where it sees the
// host function that launches it.)
#pragma once
#include <math.h>

#include "common.h"

namespace r4r {

constexpr int TOPK_MAX_K = 128;
constexpr int64_t TOPK_MAX_CHUNK = (int64_t)1 << 30;
constexpr int TOPK_TARGET_WAVES = 4096;      // 256 CUs x 16 waves
constexpr int64_t TOPK_MIN_CHUNK = 512;      // below this the partial lists cost more than the scan saves
constexpr int MERGE_THREADS = 256;

// a is ahead of b in the result order
template <class IdT>
__device__ __forceinline__ bool ahead(float sa, IdT ia, float sb, IdT ib) { return sa > sb || (sa == sb && ia < ib); }

template <class IdT> struct fill_id;
template <> struct fill_id<int> { static constexpr int value = 0x7fffffff; };
template <> struct fill_id<int64_t> { static constexpr int64_t value = 0x7fffffffffffffffLL; };

// All 64 lanes of one wave insert (s, i) into the sorted list sc / id of K <= 128 slots (two per lane); unused slots hold
// (-inf, fill_id): never ahead of a real entry, so the list needs no count and its K-th score -- what a newcomer has to
// beat, -inf while there is room -- is sc[K - 1].  Returns that score as it is after the call.  One LDS round trip:
// every lane reads its slots, a ballot gives the position, the tail moves up by one out of registers.
template <class IdT>
__device__ __forceinline__ float list_insert(float *sc, IdT *id, int K, float s, IdT i, int lane) {
    const int p0 = lane, p1 = lane + 64;
    float e0 = -INFINITY, e1 = -INFINITY;
    IdT i0 = fill_id<IdT>::value, i1 = fill_id<IdT>::value;
    if (p0 < K) { e0 = sc[p0]; i0 = id[p0]; }
    if (p1 < K) { e1 = sc[p1]; i1 = id[p1]; }
    const bool b0 = p0 < K && ahead<IdT>(e0, i0, s, i);
    const bool b1 = p1 < K && ahead<IdT>(e1, i1, s, i);
    const int pos = __popcll(__ballot(b0)) + __popcll(__ballot(b1));
    if (pos >= K) return lane_value(K > 64 ? e1 : e0, (K - 1) & 63);          // (wave-uniform) not among the K best
    wave_lds_fence();
    if (p0 < K && !b0 && p0 + 1 < K) { sc[p0 + 1] = e0; id[p0 + 1] = i0; }
    if (p1 < K && !b1 && p1 + 1 < K) { sc[p1 + 1] = e1; id[p1 + 1] = i1; }
    if (lane == 0) { sc[pos] = s; id[pos] = i; }
    wave_lds_fence();
    if (pos == K - 1) return s;
    return lane_value(K - 2 >= 64 ? e1 : e0, (K - 2) & 63);                     // the old entry K - 2 is the new K - 1
}

// ---------------------------------------------------------------------------------------------------------------------
// Around the candidate loop of a scan (one wave per workgroup)

// Workgroup blockIdx.x = (tile of queries or pairs) x (chunk [c_begin, c_end) of candidates); consecutive workgroups are
// the tiles of ONE chunk
struct ChunkGeom {
    int64_t tile, part, first, c_begin, c_end;                 // first: the tile's first query (pair)
    __device__ __forceinline__ int c_len() const { return (int)(c_end - c_begin); }       // (chunk <= 2^30)
};
__device__ __forceinline__ ChunkGeom chunk_geom(int64_t tiles, int tile_width, int64_t chunk, int64_t n_c) {
    ChunkGeom g;
    g.tile = blockIdx.x % tiles;
    g.part = blockIdx.x / tiles;
    g.first = g.tile * tile_width;
    g.c_begin = g.part * chunk;
    g.c_end = (g.c_begin + chunk < n_c) ? g.c_begin + chunk : n_c;
    return g;
}

// candidate ci is in query row u's sorted exclusion list (never, without lists)
__device__ __forceinline__ bool is_excluded(const int64_t *excl_off, const int64_t *excl_ids, int64_t u, int64_t ci) {
    if (excl_off == nullptr) return false;
    int64_t lo = excl_off[u], hi = excl_off[u + 1];
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (excl_ids[mid] < ci) lo = mid + 1; else hi = mid;
    }
    return lo < end && excl_ids[lo] == ci;
}

// ---------------------------------------------------------------------------------------------------------------------
// The scalar kernels, over a score head

// score(u, i) of explicit pairs
template <class Head>
__global__ void pair_kernel(Head h, const int64_t *__restrict__ qi, const int64_t *__restrict__ ci, int64_t n,
                            float *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    out[p] = h.score(qi[p], ci[p]);
}

// One thread per pair: the target's score -> out_score[p]; out_rank[p] = 0, or -1 for a target whose own score is -inf
// or NaN (never touched again)
template <class Head>
__global__ void rank_target_kernel(Head h, const int64_t *__restrict__ qi, const int64_t *__restrict__ ti, int64_t n,
                                   float *__restrict__ out_score, int64_t *__restrict__ out_rank) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float s = h.score(qi[p], ti[p]);
    out_score[p] = s;
    out_rank[p] = s > -INFINITY ? 0 : -1;                      // (false for NaN)
}

// Only with exclusions: the rank scan counted the excluded ids too.  One wave per pair recomputes the scalar chain of its
// query row's excluded ids and subtracts those that were ahead.  Exact, because a score's bits depend on its own pair
// only.
template <class Head>
__global__ __launch_bounds__(256) void rank_excl_kernel(Head h, const int64_t *__restrict__ qi,
                                                        const int64_t *__restrict__ ti, int64_t n_p,
                                                        const int64_t *__restrict__ excl_off,
                                                        const int64_t *__restrict__ excl_ids,
                                                        const float *__restrict__ t_score, int64_t *out_rank) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    if (p >= n_p) return;
    const float st = t_score[p];
    if (!(st > -INFINITY)) return;                            // a pair at -1 keeps its -1
    const int64_t u = qi[p], t = ti[p];
    const int64_t lo = excl_off[u], hi = excl_off[u + 1];
    const float qb = h.q_bias_of(u);
    int n = 0;
    for (int64_t e0 = lo; e0 < hi; e0 += 64) {
        const int64_t e = e0 + lane;
        if (e >= hi) continue;
        const int64_t i = excl_ids[e];
        if (i < 0 || i >= h.n_c || i == t) continue;
        n += ahead<int64_t>(h.score(u, i, qb), i, st, t) ? 1 : 0;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) n += __shfl_xor(n, m);
    if (lane == 0 && n > 0)
        atomicAdd(reinterpret_cast<unsigned long long *>(out_rank + p), (unsigned long long)(-(int64_t)n));
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side

// the chunk a call over n queries (pairs) in tiles of `tile` runs with: the caller's, or one that gives every CU its waves
inline int64_t resolve_chunk(int64_t n, int64_t n_c, int64_t chunk, int tile) {
    if (chunk > 0) return chunk;
    const int64_t tiles = cdiv(n, tile);
    int64_t parts = cdiv(TOPK_TARGET_WAVES, tiles > 0 ? tiles : 1);
    const int64_t most = cdiv(n_c, TOPK_MIN_CHUNK);
    if (parts > most) parts = most;
    if (parts < 1) parts = 1;
    return cdiv(cdiv(n_c, parts), 64) * 64;
}

// r4r_topk_*_ws_bytes: the partial lists [n_q, parts, K] of (score, id); nothing for a single chunk
inline size_t lists_ws_bytes(int64_t n_q, int64_t n_c, int K, int64_t chunk, int tile) {
    if (n_q <= 0 || n_c <= 0 || K < 1 || K > TOPK_MAX_K || chunk < 0) return 0;
    const int64_t parts = cdiv(n_c, resolve_chunk(n_q, n_c, chunk, tile));
    if (parts <= 1) return 0;
    return (size_t)n_q * (size_t)parts * (size_t)K * (sizeof(float) + sizeof(int64_t));
}

template <class Head>
inline bool head_rows(const Head &h) { return h.width() == 0 || (h.q != nullptr && h.c != nullptr); }

// The refusals of r4r_topk_<form> in fn's name.  *work = false: nothing to rank, nothing to enqueue, outputs untouched.
template <class Head>
int topk_check(const char *fn, const Head &h, int64_t n_q, const int64_t *excl_off, const int64_t *excl_ids, int K,
               int64_t chunk, const int64_t *out_ids, const float *out_scores, bool *work) {
    *work = false;
    R4R_REQUIRE(K >= 1 && K <= TOPK_MAX_K, "%s: K = %d outside 1 .. %d", fn, K, TOPK_MAX_K);
    if (const int rc = h.ranges(fn)) return rc;
    R4R_REQUIRE(n_q >= 0 && h.n_c >= 0, "%s: negative n_q or n_c", fn);
    R4R_REQUIRE(chunk >= 0 && chunk <= TOPK_MAX_CHUNK, "%s: chunk = %lld outside 0 .. 2^30", fn, (long long)chunk);
    R4R_REQUIRE((excl_off == nullptr) == (excl_ids == nullptr), "%s: excl_off and excl_ids go together (both or neither)", fn);
    R4R_REQUIRE(n_q == 0 || (out_ids != nullptr && out_scores != nullptr), "%s: null output", fn);
    R4R_REQUIRE(n_q < ((int64_t)1 << 31), "%s: n_q = %lld too large", fn, (long long)n_q);
    R4R_REQUIRE(h.c_stride >= h.width(), "%s: c_stride = %lld below %s = %d", fn, (long long)h.c_stride, Head::width_name,
                h.width());
    if (n_q == 0 || h.n_c == 0) return R4R_OK;
    if (const int rc = h.weights(fn)) return rc;
    R4R_REQUIRE(head_rows(h), "%s: null q or c with %s > 0", fn, Head::width_name);
    *work = true;
    return R4R_OK;
}

// The refusals of r4r_pair_<form>.  *work = false: no pairs.
template <class Head>
int pair_check(const char *fn, const Head &h, int64_t n_q, const int64_t *q_idx, const int64_t *c_idx, int64_t n,
               const float *out, bool *work) {
    *work = false;
    if (const int rc = h.ranges(fn)) return rc;
    R4R_REQUIRE(n >= 0 && n_q >= 0 && h.n_c >= 0, "%s: negative size", fn);
    if (n == 0) return R4R_OK;
    R4R_REQUIRE(n_q > 0 && h.n_c > 0, "%s: pairs into an empty table", fn);
    R4R_REQUIRE(h.c_stride >= h.width(), "%s: c_stride = %lld below %s = %d", fn, (long long)h.c_stride, Head::width_name,
                h.width());
    if (const int rc = h.weights(fn)) return rc;
    R4R_REQUIRE(q_idx != nullptr && c_idx != nullptr && out != nullptr && head_rows(h), "%s: null pointer", fn);
    R4R_REQUIRE(cdiv(n, 256) < ((int64_t)1 << 31), "%s: n = %lld exceeds the grid", fn, (long long)n);
    *work = true;
    return R4R_OK;
}

// The refusals of r4r_rank_<form>.  *work = false: nothing to rank, nothing to enqueue, outputs untouched.
template <class Head>
int rank_check(const char *fn, const Head &h, int64_t n_q, const int64_t *q_idx, const int64_t *t_idx, int64_t n_p,
               const int64_t *excl_off, const int64_t *excl_ids, int64_t chunk, const int64_t *out_rank,
               const float *out_score, bool *work) {
    *work = false;
    if (const int rc = h.ranges(fn)) return rc;
    R4R_REQUIRE(n_p >= 0 && n_q >= 0 && h.n_c >= 0, "%s: negative n_p, n_q or n_c", fn);
    R4R_REQUIRE(chunk >= 0 && chunk <= TOPK_MAX_CHUNK, "%s: chunk = %lld outside 0 .. 2^30", fn, (long long)chunk);
    R4R_REQUIRE((excl_off == nullptr) == (excl_ids == nullptr), "%s: excl_off and excl_ids go together (both or neither)", fn);
    R4R_REQUIRE(h.c_stride >= h.width(), "%s: c_stride = %lld below %s = %d", fn, (long long)h.c_stride, Head::width_name,
                h.width());
    R4R_REQUIRE(n_p == 0 || (out_rank != nullptr && out_score != nullptr), "%s: null output", fn);
    if (n_p == 0 || h.n_c == 0) return R4R_OK;
    R4R_REQUIRE(n_q > 0, "%s: pairs into an empty query table", fn);
    if (const int rc = h.weights(fn)) return rc;
    R4R_REQUIRE(q_idx != nullptr && t_idx != nullptr && head_rows(h), "%s: null pointer (q_idx, t_idx, or q / c with %s > 0)",
                fn, Head::width_name);
    *work = true;
    return R4R_OK;
}

// How a call is cut into workgroups: chunks of `chunk` candidates x tiles of queries (pairs)
struct ChunkPlan {
    int64_t chunk, parts, tiles;
};
// ... and where the scan of a top-K call writes: the outputs themselves for a single chunk, else the workspace's
// partial lists
struct ListsPlan : ChunkPlan {
    float *scan_scores;       // [n_q, parts, K]
    int64_t *scan_ids;
};

// chunk_tile: the tile width the chunk rule (and the form's ws_bytes) counts with, tile: the one the scan runs with
inline int topk_plan(const char *fn, int64_t n_q, int64_t n_c, int K, int64_t chunk, int chunk_tile, int tile, void *ws,
                     size_t ws_bytes, int64_t *out_ids, float *out_scores, ListsPlan *p) {
    p->chunk = resolve_chunk(n_q, n_c, chunk, chunk_tile);
    p->parts = cdiv(n_c, p->chunk);
    p->tiles = cdiv(n_q, tile);
    R4R_REQUIRE(p->parts * p->tiles < ((int64_t)1 << 31), "%s: %lld chunks x %lld query tiles exceed the grid", fn,
                (long long)p->parts, (long long)p->tiles);
    const size_t need = lists_ws_bytes(n_q, n_c, K, chunk, chunk_tile);
    if (need > 0 && (ws == nullptr || ws_bytes < need)) {
        set_error("%s: workspace %zu < %zu bytes", fn, ws_bytes, need);
        return R4R_ERR_WORKSPACE;
    }
    if (p->parts == 1) {
        p->scan_scores = out_scores;
        p->scan_ids = out_ids;
    } else {
        p->scan_ids = reinterpret_cast<int64_t *>(ws);
        p->scan_scores = reinterpret_cast<float *>(p->scan_ids + (size_t)n_q * p->parts * K);
    }
    return R4R_OK;
}

inline int rank_plan(const char *fn, int64_t n_p, int64_t n_c, int64_t chunk, int chunk_tile, int tile, ChunkPlan *p) {
    p->chunk = resolve_chunk(n_p, n_c, chunk, chunk_tile);
    p->parts = cdiv(n_c, p->chunk);
    p->tiles = cdiv(n_p, tile);
    R4R_REQUIRE(p->parts * p->tiles < ((int64_t)1 << 31) && cdiv(n_p, 4) < ((int64_t)1 << 31),
                "%s: %lld chunks x %lld pair tiles exceed the grid", fn, (long long)p->parts, (long long)p->tiles);
    return R4R_OK;
}

// topk.hip: enqueue topk_merge_kernel over partial lists ps / pi [n_q, parts, K] -> out_ids / out_scores [n_q, K]
int topk_launch_merge(const float *ps, const int64_t *pi, int64_t n_q, int64_t parts, int K, int64_t *out_ids,
                      float *out_scores, hipStream_t st);

// after the scan of a top-K call (rc: its launch): merge the chunks' partial lists, unless the scan wrote the result
inline int topk_finish(const ListsPlan &p, int rc, int64_t n_q, int K, int64_t *out_ids, float *out_scores, hipStream_t st) {
    if (rc != R4R_OK || p.parts == 1) return rc;
    return topk_launch_merge(p.scan_scores, p.scan_ids, n_q, p.parts, K, out_ids, out_scores, st);
}

template <class Head>
int launch_pairs(const Head &h, const int64_t *q_idx, const int64_t *c_idx, int64_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(pair_kernel<Head>, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, h, q_idx, c_idx, n, out);
    return check_launch("pair_kernel");
}

template <class Head>
int launch_rank_targets(const Head &h, const int64_t *q_idx, const int64_t *t_idx, int64_t n_p, float *out_score,
                        int64_t *out_rank, hipStream_t st) {
    hipLaunchKernelGGL(rank_target_kernel<Head>, dim3((unsigned)cdiv(n_p, 256)), dim3(256), 0, st, h, q_idx, t_idx, n_p,
                       out_score, out_rank);
    return check_launch("rank_target_kernel");
}

// (rc: the rank scan's launch; without exclusions there is nothing to correct)
template <class Head>
int rank_finish(const Head &h, int rc, const int64_t *q_idx, const int64_t *t_idx, int64_t n_p, const int64_t *excl_off,
                const int64_t *excl_ids, const float *t_score, int64_t *out_rank, hipStream_t st) {
    if (rc != R4R_OK || excl_off == nullptr) return rc;
    hipLaunchKernelGGL(rank_excl_kernel<Head>, dim3((unsigned)cdiv(n_p, 4)), dim3(256), 0, st, h, q_idx, t_idx, n_p, excl_off,
                       excl_ids, t_score, out_rank);
    return check_launch("rank_excl_kernel");
}

}  // namespace r4r

// The stream of the single-wave, weight-resident MFMA scans (topk_hmlp.hip: r4r_*_hmlp, topk_rfm.hip: r4r_*_rfm): one
// WAVE per workgroup = (tile of QT queries or pairs) x (chunk of candidates), the head's A fragments in registers for the
// whole chunk, 16 candidates per slab with the next slab's loads in flight, no barrier.  Written once here: the slab, the
// two argument structs, the top-K scan, the rank scan, their launches and the host sequence of the three entry points.
// A form's file keeps its score chain: the scalar chain of a pair, the head (topk_device.h), the WAVE, the dispatch
// table of its classes.
//
// A Wave is what one wave keeps for its whole chunk and how it scores a slab:
//   typedef ... Head;  static constexpr int KT, QT    the form's head; MFMAs over the input width (width <= 4 KT);
//                                                     queries (pairs) per wave
//   init(head, lane)                                  the A fragments and the epilogue's vectors of the head, row = lane
//                                                     & 15, kq = lane >> 4, jo[KT] = the column lane (., kq) reads for
//                                                     MFMA t, clamped into the row
//   query(head, src, exists, qf[KT])                  the query row `src` as its B-fragment operand; zeros for a row that
//                                                     does not exist
//   scores(bf[KT], qf[QT][KT], cb, sv[QT])            the slab's c registers against QT queries -> the score of
//                                                     candidate `row` per query, without the query's bias
// The kernels are templates over the WHOLE wave type, and every inner piece -- clearing and writing back the lists, the
// survivor loop, (ts, trel) of a ranked pair, the wave sum of its counters -- is still written out in them: that leaves
// the instructions of all 64 instantiations as they were (profiles/topk_mfma_shared_isa.txt).  Helpers for those pieces
// moved the register allocation of a whole scan (profiles/topk_shared_isa.txt), and a common base struct for the two
// waves' wf / jo / query changed all 32 streaming kernels (profiles/topk_mfma_shared_isa.txt): the wave structs stay
// whole, each in its form's file.
#pragma once
#include <math.h>

#include "common.h"
#include "slate_device.h"
#include "topk_device.h"

namespace r4r {

// the B fragments of one slab in flight: c[slab + row][4 t + kq] and the row's bias
template <class Head, int KT>
struct MfmaSlab {
    float bn[KT], cbn;

    __device__ __forceinline__ void clear() {
        cbn = 0.f;
#pragma unroll
        for (int t = 0; t < KT; ++t) bn[t] = 0.f;
    }
    // Unconditional loads from clamped addresses: a column past D reads column D - 1 and is zeroed in `take`, a row of
    // the NEXT chunk is read and ignored, a row past the table reads the table's last row.
    __device__ __forceinline__ void load(const Head &a, const int (&jo)[KT], int64_t i) {
        const int64_t ic = i < a.n_c ? i : a.n_c - 1;
        const float *src = a.c + ic * a.c_stride;
        if (a.D > 0) {
#pragma unroll
            for (int t = 0; t < KT; ++t) bn[t] = src[jo[t]];
        }
        if (a.c_bias != nullptr) cbn = a.c_bias[ic];
    }
    __device__ __forceinline__ void take(int D, int kq, float (&bf)[KT], float &cb) const {
        cb = cbn;
#pragma unroll
        for (int t = 0; t < KT; ++t) bf[t] = (4 * t + kq < D) ? bn[t] : 0.f;
    }
};

template <class Head>
struct MfmaScanArgs {
    Head h;
    const int64_t *excl_off, *excl_ids;
    float *out_scores;        // [n_q, parts, K]
    int64_t *out_ids;
    int64_t n_q, chunk, parts, tiles;
    int K;
};

// Scores are never written: each is compared with its query's K-th best, survivors go through list_insert, the partial
// lists have r4r_topk_dot's workspace layout
template <class Wave>
__global__ __launch_bounds__(64) void mfma_scan_kernel(MfmaScanArgs<typename Wave::Head> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mfma_lds[];
    constexpr int KT = Wave::KT, QT = Wave::QT;
    const int K = a.K, D = a.h.D;
    float *sc = reinterpret_cast<float *>(mfma_lds);           // [QT][K]
    int *id = reinterpret_cast<int *>(sc + QT * K);            // [QT][K]  candidate - chunk begin

    const int lane = threadIdx.x;
    const ChunkGeom g = chunk_geom(a.tiles, QT, a.chunk, a.h.n_c);
    const int64_t u0 = g.first, c_begin = g.c_begin, c_end = g.c_end;

    for (int i = lane; i < QT * K; i += 64) { sc[i] = -INFINITY; id[i] = fill_id<int>::value; }

    Wave wv;
    wv.init(a.h, lane);
    const int row = wv.row, kq = wv.kq;
    float qf[QT][KT], qb[QT], thr[QT];                         // qb, thr: wave-uniform
#pragma unroll
    for (int s = 0; s < QT; ++s) {
        const int64_t u = u0 + s;
        const bool exists = u < a.n_q;
        const int64_t uc = exists ? u : a.n_q - 1;
        wv.query(a.h, a.h.q + uc * D, exists, qf[s]);
        qb[s] = a.h.q_bias != nullptr ? a.h.q_bias[uc] : 0.f;
        thr[s] = exists ? -INFINITY : INFINITY;                // rows past n_q never survive
    }
    wave_lds_fence();

    MfmaSlab<typename Wave::Head, KT> nx;
    float bf[KT], cb;
    nx.clear();
    if (c_begin < c_end) nx.load(a.h, wv.jo, c_begin + row);
    nx.take(D, kq, bf, cb);
    for (int64_t base = c_begin; base < c_end; base += 16) {
        if (base + 16 < c_end) nx.load(a.h, wv.jo, base + 16 + row);
        float sv[QT];
        wv.scores(bf, qf, cb, sv);
        const bool live = kq == 0 && base + row < c_end;       // one lane per candidate offers it
        bool any = false;
#pragma unroll
        for (int s = 0; s < QT; ++s) {
            sv[s] = sv[s] + qb[s];
            any |= live && sv[s] > thr[s];                     // (false for a NaN score)
        }
        if (__ballot(any) != 0) {
            // survivors, one at a time (wave-uniform control flow from here on)
#pragma unroll
            for (int s = 0; s < QT; ++s) {
                unsigned long long m = __ballot(live && sv[s] > thr[s]);
                while (m) {
                    const int src = __builtin_ctzll(m);
                    m &= m - 1;
                    const float v = lane_value(sv[s], src);
                    const int64_t ci = base + src;             // (src < 16: a lane of kq == 0)
                    if (!(v > thr[s])) continue;               // (an earlier survivor raised the bar)
                    if (is_excluded(a.excl_off, a.excl_ids, u0 + s, ci)) continue;
                    thr[s] = list_insert<int>(sc + s * K, id + s * K, K, v, (int)(ci - c_begin), lane);
                }
            }
        }
        nx.take(D, kq, bf, cb);
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
// r4r_rank_<form>: r4r_rank_dot's three launches over the form's chain.
//   A  rank_target_kernel<Head>       one thread per pair: the scalar chain -> out_score[p]; out_rank[p] = 0, or -1 for a
//                                     target whose own score is -inf or NaN (never touched again)
//   B  mfma_rank_scan_kernel          the scan's stream over a tile of QT PAIRS (query rows gathered through q_idx) and a
//                                     chunk of candidates; every score is compared with the pair's target in registers
//                                     and counted; one 64-bit integer atomic per (pair, chunk)
//   C  rank_excl_kernel<Head>         only with exclusions: B counted the excluded ids too; one wave per pair recomputes
//                                     the scalar chain of its query row's excluded ids and subtracts those that were ahead
// (A and C: topk_device.h.)
template <class Head>
struct MfmaRankArgs {
    Head h;
    const int64_t *q_idx, *t_idx;
    const float *t_score;     // out_score, written by launch A
    int64_t *out_rank;
    int64_t n_p, chunk, tiles;
};

template <class Wave>
__global__ __launch_bounds__(64) void mfma_rank_scan_kernel(MfmaRankArgs<typename Wave::Head> a) {
    constexpr int KT = Wave::KT, PT = Wave::QT;
    const int D = a.h.D;
    const int lane = threadIdx.x;
    const ChunkGeom g = chunk_geom(a.tiles, PT, a.chunk, a.h.n_c);
    const int64_t p0 = g.first, c_begin = g.c_begin, c_end = g.c_end;
    const int c_len = g.c_len();

    Wave wv;
    wv.init(a.h, lane);
    const int row = wv.row, kq = wv.kq;
    // Of each pair: its query row, its query bias, its target's score and its target's id relative to the chunk (-1:
    // before it, so no tie is ahead; INT_MAX: behind it, so every tie is).  A pair past n_p or at -1 waits for a score
    // above +inf: it counts nothing.  (All wave-uniform.)
    float qf[PT][KT], qb[PT], ts[PT];
    int trel[PT], cnt[PT];
#pragma unroll
    for (int s = 0; s < PT; ++s) {
        const int64_t p = p0 + s;
        const bool exists = p < a.n_p;
        const int64_t pc = exists ? p : a.n_p - 1;
        const int64_t u = a.q_idx[pc];
        wv.query(a.h, a.h.q + u * D, exists, qf[s]);
        qb[s] = a.h.q_bias != nullptr ? a.h.q_bias[u] : 0.f;
        const float st = a.t_score[pc];
        const int64_t d = a.t_idx[pc] - c_begin;
        const bool ranked = exists && st > -INFINITY;          // (false for NaN)
        ts[s] = ranked ? st : INFINITY;
        trel[s] = !ranked || d < 0 ? -1 : (d > 0x7fffffff ? 0x7fffffff : (int)d);
        cnt[s] = 0;
    }

    MfmaSlab<typename Wave::Head, KT> nx;
    float bf[KT], cb;
    nx.clear();
    if (c_begin < c_end) nx.load(a.h, wv.jo, c_begin + row);
    nx.take(D, kq, bf, cb);
    for (int64_t base = c_begin; base < c_end; base += 16) {
        if (base + 16 < c_end) nx.load(a.h, wv.jo, base + 16 + row);
        float sv[PT];
        wv.scores(bf, qf, cb, sv);
        const int rel = (int)(base - c_begin) + row;
        const bool live = kq == 0 && rel < c_len;              // one lane per candidate counts it
#pragma unroll
        for (int s = 0; s < PT; ++s)
            cnt[s] += (live && ahead<int>(sv[s] + qb[s], rel, ts[s], trel[s])) ? 1 : 0;     // (false for a NaN score)
        nx.take(D, kq, bf, cb);
    }

    // lane s adds pair s's count over the wave to its rank -- one atomic instruction per wave
    int mine = 0;
#pragma unroll
    for (int s = 0; s < PT; ++s) {
        int v = cnt[s];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
        if (lane == s) mine = v;
    }
    // (mine > 0 only for a pair below n_p whose target is ranked: the others wait for +inf)
    if (lane < PT && mine > 0)
        atomicAdd(reinterpret_cast<unsigned long long *>(a.out_rank + p0 + lane), (unsigned long long)mine);
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side.  `kernel`: what a launch error calls the form's instantiation.

template <class Wave>
int launch_mfma_scan(const char *kernel, const MfmaScanArgs<typename Wave::Head> &a, hipStream_t st) {
    const size_t lds = (size_t)Wave::QT * (size_t)a.K * 8;
    hipLaunchKernelGGL((mfma_scan_kernel<Wave>), dim3((unsigned)(a.parts * a.tiles)), dim3(64), lds, st, a);
    return check_launch(kernel);
}

template <class Wave>
int launch_mfma_rank(const char *kernel, const MfmaRankArgs<typename Wave::Head> &a, int64_t parts, hipStream_t st) {
    hipLaunchKernelGGL((mfma_rank_scan_kernel<Wave>), dim3((unsigned)(parts * a.tiles)), dim3(64), 0, st, a);
    return check_launch(kernel);
}

// The three entry points of a form.  fn: the entry point's name in its messages; chunk_tile: the tile width the chunk
// rule and the form's ws_bytes count with, tile: the one the class that serves this head runs with; dispatch: the
// form's table -> launch_mfma_scan / launch_mfma_rank of that class.
template <class Head>
int mfma_topk_call(const char *fn, const Head &h, int chunk_tile, int tile,
                   int (*dispatch)(const MfmaScanArgs<Head> &, hipStream_t), int64_t n_q, const int64_t *excl_off,
                   const int64_t *excl_ids, int K, int64_t chunk, void *ws, size_t ws_bytes, int64_t *out_ids,
                   float *out_scores, void *stream) {
    MfmaScanArgs<Head> a;
    a.h = h;
    bool work;
    int rc = topk_check(fn, a.h, n_q, excl_off, excl_ids, K, chunk, out_ids, out_scores, &work);
    if (rc != R4R_OK || !work) return rc;
    ListsPlan p;
    rc = topk_plan(fn, n_q, h.n_c, K, chunk, chunk_tile, tile, ws, ws_bytes, out_ids, out_scores, &p);
    if (rc != R4R_OK) return rc;
    a.excl_off = excl_off; a.excl_ids = excl_ids;
    a.out_scores = p.scan_scores; a.out_ids = p.scan_ids;
    a.n_q = n_q; a.chunk = p.chunk; a.parts = p.parts; a.tiles = p.tiles; a.K = K;
    hipStream_t st = as_stream(stream);
    return topk_finish(p, dispatch(a, st), n_q, K, out_ids, out_scores, st);
}

template <class Head>
int mfma_pair_call(const char *fn, const Head &h, int64_t n_q, const int64_t *q_idx, const int64_t *c_idx, int64_t n,
                   float *out, void *stream) {
    bool work;
    const int rc = pair_check(fn, h, n_q, q_idx, c_idx, n, out, &work);
    if (rc != R4R_OK || !work) return rc;
    return launch_pairs(h, q_idx, c_idx, n, out, as_stream(stream));
}

template <class Head>
int mfma_rank_call(const char *fn, const Head &h, int chunk_tile, int tile,
                   int (*dispatch)(const MfmaRankArgs<Head> &, int64_t, hipStream_t), int64_t n_q, const int64_t *q_idx,
                   const int64_t *t_idx, int64_t n_p, const int64_t *excl_off, const int64_t *excl_ids, int64_t chunk,
                   int64_t *out_rank, float *out_score, void *stream) {
    MfmaRankArgs<Head> a;
    a.h = h;
    bool work;
    int rc = rank_check(fn, a.h, n_q, q_idx, t_idx, n_p, excl_off, excl_ids, chunk, out_rank, out_score, &work);
    if (rc != R4R_OK || !work) return rc;
    ChunkPlan p;
    rc = rank_plan(fn, n_p, h.n_c, chunk, chunk_tile, tile, &p);
    if (rc != R4R_OK) return rc;
    a.q_idx = q_idx; a.t_idx = t_idx;
    a.t_score = out_score; a.out_rank = out_rank;
    a.n_p = n_p; a.chunk = p.chunk; a.tiles = p.tiles;
    hipStream_t st = as_stream(stream);
    rc = launch_rank_targets(a.h, q_idx, t_idx, n_p, out_score, out_rank, st);
    if (rc != R4R_OK) return rc;
    return rank_finish(a.h, dispatch(a, p.parts, st), q_idx, t_idx, n_p, excl_off, excl_ids, out_score, out_rank, st);
}

// The two slate calls of a form (slate_device.h): scalar chains over the head, no stream and no dispatch table
template <class Head>
int mfma_slate_topk_call(const char *fn, const Head &h, int64_t n_q, const int64_t *q_idx, const int64_t *slate_off,
                         const int64_t *slate_ids, int64_t n_s, int64_t max_len, const int64_t *excl_off,
                         const int64_t *excl_ids, int K, void *ws, size_t ws_bytes, int64_t *out_ids, float *out_scores,
                         void *stream) {
    return slate_topk_call(fn, h, n_q, q_idx, slate_off, slate_ids, n_s, max_len, excl_off, excl_ids, K, ws, ws_bytes,
                           out_ids, out_scores, stream);
}

template <class Head>
int mfma_slate_rank_call(const char *fn, const Head &h, int64_t n_q, const int64_t *q_idx, const int64_t *t_idx,
                         const int64_t *slate_off, const int64_t *slate_ids, int64_t n_p, int64_t max_len,
                         const int64_t *excl_off, const int64_t *excl_ids, int64_t *out_rank, float *out_score,
                         void *stream) {
    return slate_rank_call(fn, h, n_q, q_idx, t_idx, slate_off, slate_ids, n_p, max_len, excl_off, excl_ids, out_rank,
                           out_score, stream);
}

}  // namespace r4r

// Catalogue top-K and ranks over a ReLU-FM head: r4r_topk_rfm / r4r_pair_rfm / r4r_rank_rfm (include/r4r.h,
// "Catalogue recommendation: ReLU-FM heads").
//
//   x_m = fmaxf(q[u][m] + c[i][m], 0)   m < H          x_m = q[u][m] + c[i][m]   H <= m < D = H + P
//   y_j = fmaf(W[j][m], x_m, y_j)   m ascending, then y_j = y_j + b[j]                              j < M
//   e_j = fmaf(s[j], y_j, l[j])     t_g = fmaf(e_j, y_j, t_g)   over the j with ((j >> 2) & 3) == g, ascending
//   score(u, i) = ((((t_0 + t_1) + (t_2 + t_3)) + c_bias[i]) + q_bias[u])
//
// topk_hmlp.hip's scan with two changes: the B operand is relu(q + c) (plain q + c behind column H) instead of q * c, and
// the epilogue is y (s y + l) -- signed squares and one linear term, an FM of a linear image -- instead of w relu(y + b).
// Launch 1, rfm_scan_kernel: one WAVE per workgroup = (tile of QT queries) x (chunk of candidates), no barrier.
//   A  lane l supplies W[16 mt + (l & 15)][4 t + (l >> 4)] for MFMA (mt, t): loaded once, kept in registers for the whole
//      chunk (at the limits 5 x 20 fragments; DESIGN.md 4.18 has the budget).
//   B  lane l loads c[slab + (l & 15)][4 t + (l >> 4)], adds its query's q[u][4 t + (l >> 4)] and takes v_max_f32 with 0
//      where the column is below H.  4 t + 3 < H: the whole step is ReLU'd, 4 t >= H: none of it (both wave-uniform, so a
//      multiple-of-4 H costs no select); the one step that straddles H selects per lane.
//   C  lane l holds y of rows 16 mt + 4 (l >> 4) + r, r = 0 .. 3, for candidate l & 15: the epilogue adds b, runs the
//      e / t chain of ITS lane group g = l >> 4 over (mt, r); two cross-lane adds (xor 16, xor 32: both orders of either
//      add give the same bits) finish the sum, then the two biases.  A row at or behind M is taken as y = 0 whatever its
//      accumulator holds (0 * inf from an overflowed x), so it adds e y = 0.
// Scores are never written: each is compared with its query's K-th best, survivors go through topk_device.h's
// list_insert, the partial lists have r4r_topk_dot's workspace layout and topk.hip's merge kernel finishes (skipped for a
// single chunk).  r4r_rank_rfm: the same stream over a tile of PAIRS with counters in place of lists.
// topk_device.h's scalar kernels (pairs, rank targets, the exclusion correction) over this file's RfmHead compute
// rfm_pair_score: the chain above written out.  v_mfma_f32_16x16x4_f32 is bitwise that chain over m (topk.hip).
#include <math.h>

#include "common.h"
#include "topk_device.h"

namespace r4r {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RFM_MAX_H = 64;
constexpr int RFM_MAX_P = 16;
constexpr int RFM_MAX_M = 80;
constexpr int RFM_CHUNK_QT = 4;    // the tile width the chunk rule and r4r_topk_rfm_ws_bytes count with
// queries (pairs, for the rank) per wave: 4, or 2 where 4 sets of accumulators and query rows beside the A fragments
// would not leave the wave its registers
constexpr int rfm_qt(int KT, int MT) { return KT * MT > 50 ? 2 : 4; }

// the scalar chain of one pair: q, c point at the pair's rows.  (g is a compile-time index: t stays in registers.)
__device__ __forceinline__ float rfm_pair_score(const float *q, const float *c, const float *W, const float *b, const float *s,
                                                const float *l, int H, int D, int M, float cb, float qb) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < M; j0 += 16) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 4 * g + r;
                if (j >= M) break;
                const float *Wj = W + (size_t)j * D;
                float y = 0.f;
                for (int m = 0; m < H; ++m) y = __builtin_fmaf(Wj[m], __builtin_fmaxf(q[m] + c[m], 0.f), y);
                for (int m = H; m < D; ++m) y = __builtin_fmaf(Wj[m], q[m] + c[m], y);
                y = y + (b != nullptr ? b[j] : 0.f);
                const float e = __builtin_fmaf(s[j], y, l[j]);
                t[g] = __builtin_fmaf(e, y, t[g]);
            }
        }
    }
    return (((t[0] + t[1]) + (t[2] + t[3])) + cb) + qb;
}

// The head of this form (topk_device.h); the two streams read its fields
struct RfmHead {
    const float *q, *q_bias, *c, *c_bias, *W, *b, *s, *l;
    int64_t n_c, c_stride;
    int H, P, M, D;           // D = H + P

    __device__ __forceinline__ float q_bias_of(int64_t u) const { return q_bias ? q_bias[u] : 0.f; }
    __device__ __forceinline__ float score(int64_t u, int64_t i, float qb) const {
        return rfm_pair_score(q + u * D, c + i * c_stride, W, b, s, l, H, D, M, c_bias ? c_bias[i] : 0.f, qb);
    }
    __device__ __forceinline__ float score(int64_t u, int64_t i) const { return score(u, i, q_bias_of(u)); }

    static constexpr const char *width_name = "H + P";
    int width() const { return D; }
    int ranges(const char *fn) const {
        R4R_REQUIRE(H >= 0 && H <= RFM_MAX_H, "%s: H = %d outside 0 .. %d", fn, H, RFM_MAX_H);
        R4R_REQUIRE(P >= 0 && P <= RFM_MAX_P, "%s: P = %d outside 0 .. %d", fn, P, RFM_MAX_P);
        R4R_REQUIRE(M >= 0 && M <= RFM_MAX_M, "%s: M = %d outside 0 .. %d", fn, M, RFM_MAX_M);
        return R4R_OK;
    }
    int weights(const char *fn) const {
        R4R_REQUIRE(M == 0 || (W != nullptr && s != nullptr && l != nullptr), "%s: null W, s or l with M > 0", fn);
        return R4R_OK;
    }
};

// What a wave keeps for its whole chunk: the head (A fragments; b, s and l in the accumulator layout) and the column of
// each B fragment.  KT: MFMAs over the input width (D <= 4 KT), MT: 16-row tiles of y (M <= 16 MT), QT: queries per wave.
template <int KT, int MT, int QT>
struct RfmWave {
    float wf[MT][KT];          // W[16 mt + row][4 t + kq]; zero beyond M and beyond D
    float bj[MT][4], sj[MT][4], lj[MT][4];     // b / s / l of row 16 mt + 4 kq + r; zero beyond M (and for a NULL b)
    int jo[KT];                // the column lane (., kq) reads for MFMA t, clamped into the row
    int row, kq, H, mleft;     // mleft = M - 4 kq: this lane's accumulator (mt, r) is a row below M iff 16 mt + r < mleft

    __device__ __forceinline__ void init(const RfmHead &a, int lane) {
        row = lane & 15;
        kq = lane >> 4;
        H = a.H;
        const int D = a.D, M = a.M;
        mleft = M - 4 * kq;
#pragma unroll
        for (int t = 0; t < KT; ++t) jo[t] = (4 * t + kq < D) ? 4 * t + kq : (D > 0 ? D - 1 : 0);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int j = 16 * mt + row;
            const int jc = j < M ? j : (M > 0 ? M - 1 : 0);
#pragma unroll
            for (int t = 0; t < KT; ++t) wf[mt][t] = 0.f;
            if (D > 0 && M > 0) {
#pragma unroll
                for (int t = 0; t < KT; ++t) wf[mt][t] = a.W[(size_t)jc * D + jo[t]];
            }
#pragma unroll
            for (int t = 0; t < KT; ++t) wf[mt][t] = (j < M && 4 * t + kq < D) ? wf[mt][t] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = 16 * mt + 4 * kq + r;
                const int ec = e < M ? e : (M > 0 ? M - 1 : 0);
                float bv = 0.f, sv = 0.f, lv = 0.f;
                if (M > 0) {
                    sv = a.s[ec];
                    lv = a.l[ec];
                    if (a.b != nullptr) bv = a.b[ec];
                }
                bj[mt][r] = e < M ? bv : 0.f;
                sj[mt][r] = e < M ? sv : 0.f;
                lj[mt][r] = e < M ? lv : 0.f;
            }
        }
    }

    // the query row `src` as B-fragment addends: q[.][4 t + kq], zero beyond D (and for a row that does not exist)
    __device__ __forceinline__ void query(const RfmHead &a, const float *src, bool exists, float (&qf)[KT]) const {
#pragma unroll
        for (int t = 0; t < KT; ++t) qf[t] = 0.f;
        if (a.D > 0) {
#pragma unroll
            for (int t = 0; t < KT; ++t) qf[t] = src[jo[t]];
        }
#pragma unroll
        for (int t = 0; t < KT; ++t) qf[t] = (exists && 4 * t + kq < a.D) ? qf[t] : 0.f;
    }

    // The slab's c registers against QT queries -> sv[s], the score of candidate `row` for query s (the same in all four
    // lanes of a candidate), without the query's bias.
    __device__ __forceinline__ void scores(const float (&bf)[KT], const float (&qf)[QT][KT], float cb, float (&sv)[QT]) const {
        f32x4 acc[QT][MT];
#pragma unroll
        for (int s = 0; s < QT; ++s)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[s][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // every accumulator sees t ascending; the QT * MT chains are independent and interleave in the matrix pipe
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const bool all = 4 * t + 3 < H, none = 4 * t >= H;         // wave-uniform
#pragma unroll
            for (int s = 0; s < QT; ++s) {
                const float v = bf[t] + qf[s][t];
                const float r = __builtin_fmaxf(v, 0.f);
                const float x = all ? r : (none ? v : (4 * t + kq < H ? r : v));
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    acc[s][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[mt][t], x, acc[s][mt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int s = 0; s < QT; ++s) {
            float tg = 0.f;                                    // t_g of this lane's group g = kq
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float y = (16 * mt + r < mleft ? acc[s][mt][r] : 0.f) + bj[mt][r];
                    tg = __builtin_fmaf(__builtin_fmaf(sj[mt][r], y, lj[mt][r]), y, tg);
                }
            tg = tg + __shfl_xor(tg, 16);                      // t_0 + t_1 | t_2 + t_3
            tg = tg + __shfl_xor(tg, 32);                      // (t_0 + t_1) + (t_2 + t_3)
            sv[s] = tg + cb;
        }
    }
};

// the B fragments of one slab in flight: c[slab + row][4 t + kq] and the row's bias
template <int KT>
struct RfmSlab {
    float bn[KT], cbn;

    __device__ __forceinline__ void clear() {
        cbn = 0.f;
#pragma unroll
        for (int t = 0; t < KT; ++t) bn[t] = 0.f;
    }
    // Unconditional loads from clamped addresses: a column past D reads column D - 1 and is zeroed in `take`, a row of
    // the NEXT chunk is read and ignored, a row past the table reads the table's last row.
    __device__ __forceinline__ void load(const RfmHead &a, const int (&jo)[KT], int64_t i) {
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

struct RfmScanArgs {
    RfmHead h;
    const int64_t *excl_off, *excl_ids;
    float *out_scores;        // [n_q, parts, K]
    int64_t *out_ids;
    int64_t n_q, chunk, parts, tiles;
    int K;
};

template <int KT, int MT>
__global__ __launch_bounds__(64) void rfm_scan_kernel(RfmScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rfm_lds[];
    constexpr int QT = rfm_qt(KT, MT);
    const int K = a.K, D = a.h.D;
    float *sc = reinterpret_cast<float *>(rfm_lds);            // [QT][K]
    int *id = reinterpret_cast<int *>(sc + QT * K);            // [QT][K]  candidate - chunk begin

    const int lane = threadIdx.x;
    const ChunkGeom g = chunk_geom(a.tiles, QT, a.chunk, a.h.n_c);
    const int64_t u0 = g.first, c_begin = g.c_begin, c_end = g.c_end;

    for (int i = lane; i < QT * K; i += 64) { sc[i] = -INFINITY; id[i] = fill_id<int>::value; }

    RfmWave<KT, MT, QT> wv;
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

    RfmSlab<KT> nx;
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
// r4r_rank_rfm: r4r_rank_dot's three launches over this file's chain.
//   A  rank_target_kernel<RfmHead>    one thread per pair: the scalar chain -> out_score[p]; out_rank[p] = 0, or -1 for a
//                                     target whose own score is -inf or NaN (never touched again)
//   B  rank_rfm_scan_kernel           the scan's stream over a tile of QT PAIRS (query rows gathered through q_idx) and a
//                                     chunk of candidates; every score is compared with the pair's target in registers
//                                     and counted; one 64-bit integer atomic per (pair, chunk)
//   C  rank_excl_kernel<RfmHead>      only with exclusions: B counted the excluded ids too; one wave per pair recomputes
//                                     the scalar chain of its query row's excluded ids and subtracts those that were ahead
// (A and C: topk_device.h.)
struct RfmRankArgs {
    RfmHead h;
    const int64_t *q_idx, *t_idx;
    const float *t_score;     // out_score, written by launch A
    int64_t *out_rank;
    int64_t n_p, chunk, tiles;
};

template <int KT, int MT>
__global__ __launch_bounds__(64) void rank_rfm_scan_kernel(RfmRankArgs a) {
    constexpr int PT = rfm_qt(KT, MT);
    const int D = a.h.D;
    const int lane = threadIdx.x;
    const ChunkGeom g = chunk_geom(a.tiles, PT, a.chunk, a.h.n_c);
    const int64_t p0 = g.first, c_begin = g.c_begin, c_end = g.c_end;
    const int c_len = g.c_len();

    RfmWave<KT, MT, PT> wv;
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

    RfmSlab<KT> nx;
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

template <int KT, int MT>
int launch_rfm_scan(const RfmScanArgs &a, hipStream_t st) {
    const size_t lds = (size_t)rfm_qt(KT, MT) * (size_t)a.K * 8;
    hipLaunchKernelGGL((rfm_scan_kernel<KT, MT>), dim3((unsigned)(a.parts * a.tiles)), dim3(64), lds, st, a);
    return check_launch("rfm_scan_kernel");
}

template <int KT, int MT>
int launch_rfm_rank(const RfmRankArgs &a, int64_t parts, hipStream_t st) {
    hipLaunchKernelGGL((rank_rfm_scan_kernel<KT, MT>), dim3((unsigned)(parts * a.tiles)), dim3(64), 0, st, a);
    return check_launch("rank_rfm_scan_kernel");
}

// KT by D (2, 4, 10, 20 MFMAs over the input width), MT by M (1, 2, 3, 5 tiles of 16 rows): sixteen of each kernel.
// TransNet(++) at latent sizes 6 / 10 / 16 / 32 / 64 lands on <2 | 4, 1>, <4 | 10, 2>, <4 | 10, 2>, <10, 3>, <20, 5>.
inline int rfm_kt(int D) { return D <= 8 ? 2 : D <= 16 ? 4 : D <= 40 ? 10 : 20; }
inline int rfm_mt(int M) { return M <= 16 ? 1 : M <= 32 ? 2 : M <= 48 ? 3 : 5; }
// the queries (pairs) per wave of the instantiation that serves (D, M)
inline int rfm_tile(int D, int M) { return rfm_qt(rfm_kt(D), rfm_mt(M)); }

#define RFM_DISPATCH(FN, D, M, ...)                                                    \
    do {                                                                               \
        switch (rfm_kt(D) * 8 + rfm_mt(M)) {                                           \
        case 2 * 8 + 1: return FN<2, 1>(__VA_ARGS__);                                  \
        case 2 * 8 + 2: return FN<2, 2>(__VA_ARGS__);                                  \
        case 2 * 8 + 3: return FN<2, 3>(__VA_ARGS__);                                  \
        case 2 * 8 + 5: return FN<2, 5>(__VA_ARGS__);                                  \
        case 4 * 8 + 1: return FN<4, 1>(__VA_ARGS__);                                  \
        case 4 * 8 + 2: return FN<4, 2>(__VA_ARGS__);                                  \
        case 4 * 8 + 3: return FN<4, 3>(__VA_ARGS__);                                  \
        case 4 * 8 + 5: return FN<4, 5>(__VA_ARGS__);                                  \
        case 10 * 8 + 1: return FN<10, 1>(__VA_ARGS__);                                \
        case 10 * 8 + 2: return FN<10, 2>(__VA_ARGS__);                                \
        case 10 * 8 + 3: return FN<10, 3>(__VA_ARGS__);                                \
        case 10 * 8 + 5: return FN<10, 5>(__VA_ARGS__);                                \
        case 20 * 8 + 1: return FN<20, 1>(__VA_ARGS__);                                \
        case 20 * 8 + 2: return FN<20, 2>(__VA_ARGS__);                                \
        case 20 * 8 + 3: return FN<20, 3>(__VA_ARGS__);                                \
        default: return FN<20, 5>(__VA_ARGS__);                                        \
        }                                                                              \
    } while (0)

int dispatch_rfm_scan(const RfmScanArgs &a, hipStream_t st) { RFM_DISPATCH(launch_rfm_scan, a.h.D, a.h.M, a, st); }
int dispatch_rfm_rank(const RfmRankArgs &a, int64_t parts, hipStream_t st) {
    RFM_DISPATCH(launch_rfm_rank, a.h.D, a.h.M, a, parts, st);
}

inline RfmHead rfm_head(const float *q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                        const float *c_bias, const float *W, const float *b, const float *s, const float *l, int H, int P,
                        int M) {
    RfmHead h;
    h.q = q; h.q_bias = q_bias; h.c = c; h.c_bias = c_bias; h.W = W; h.b = b; h.s = s; h.l = l;
    h.n_c = n_c; h.c_stride = c_stride; h.H = H; h.P = P; h.M = M;
    // (out-of-range H or P: ranges() refuses before D is used)
    h.D = (H >= 0 && H <= RFM_MAX_H && P >= 0 && P <= RFM_MAX_P) ? H + P : 0;
    return h;
}

}  // namespace
}  // namespace r4r

using namespace r4r;

extern "C" size_t r4r_topk_rfm_ws_bytes(int64_t n_q, int64_t n_c, int K, int64_t chunk) {
    return lists_ws_bytes(n_q, n_c, K, chunk, RFM_CHUNK_QT);
}

extern "C" int r4r_topk_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                            const float *c_bias, const float *W, const float *b, const float *s, const float *l, int H, int P,
                            int M, const int64_t *excl_off, const int64_t *excl_ids, int K, int64_t chunk, void *ws,
                            size_t ws_bytes, int64_t *out_ids, float *out_scores, void *stream) {
    RfmScanArgs a;
    a.h = rfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, l, H, P, M);
    bool work;
    int rc = topk_check("topk_rfm", a.h, n_q, excl_off, excl_ids, K, chunk, out_ids, out_scores, &work);
    if (rc != R4R_OK || !work) return rc;
    ListsPlan p;
    rc = topk_plan("topk_rfm", n_q, n_c, K, chunk, RFM_CHUNK_QT, rfm_tile(a.h.D, M), ws, ws_bytes, out_ids, out_scores, &p);
    if (rc != R4R_OK) return rc;
    a.excl_off = excl_off; a.excl_ids = excl_ids;
    a.out_scores = p.scan_scores; a.out_ids = p.scan_ids;
    a.n_q = n_q; a.chunk = p.chunk; a.parts = p.parts; a.tiles = p.tiles; a.K = K;
    hipStream_t st = as_stream(stream);
    return topk_finish(p, dispatch_rfm_scan(a, st), n_q, K, out_ids, out_scores, st);
}

extern "C" int r4r_pair_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                            const float *c_bias, const float *W, const float *b, const float *s, const float *l, int H, int P,
                            int M, const int64_t *q_idx, const int64_t *c_idx, int64_t n, float *out, void *stream) {
    const RfmHead h = rfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, l, H, P, M);
    bool work;
    const int rc = pair_check("pair_rfm", h, n_q, q_idx, c_idx, n, out, &work);
    if (rc != R4R_OK || !work) return rc;
    return launch_pairs(h, q_idx, c_idx, n, out, as_stream(stream));
}

extern "C" int r4r_rank_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                            const float *c_bias, const float *W, const float *b, const float *s, const float *l, int H, int P,
                            int M, const int64_t *q_idx, const int64_t *t_idx, int64_t n_p, const int64_t *excl_off,
                            const int64_t *excl_ids, int64_t chunk, int64_t *out_rank, float *out_score, void *stream) {
    RfmRankArgs a;
    a.h = rfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, l, H, P, M);
    bool work;
    int rc = rank_check("rank_rfm", a.h, n_q, q_idx, t_idx, n_p, excl_off, excl_ids, chunk, out_rank, out_score, &work);
    if (rc != R4R_OK || !work) return rc;
    ChunkPlan p;
    rc = rank_plan("rank_rfm", n_p, n_c, chunk, RFM_CHUNK_QT, rfm_tile(a.h.D, M), &p);
    if (rc != R4R_OK) return rc;
    a.q_idx = q_idx; a.t_idx = t_idx;
    a.t_score = out_score; a.out_rank = out_rank;
    a.n_p = n_p; a.chunk = p.chunk; a.tiles = p.tiles;
    hipStream_t st = as_stream(stream);
    rc = launch_rank_targets(a.h, q_idx, t_idx, n_p, out_score, out_rank, st);
    if (rc != R4R_OK) return rc;
    return rank_finish(a.h, dispatch_rfm_rank(a, p.parts, st), q_idx, t_idx, n_p, excl_off, excl_ids, out_score, out_rank, st);
}

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
// Launch 1, mfma_scan_kernel<RfmWave> (topk_mfma_device.h has the stream): one WAVE per workgroup = (tile of QT queries) x
// (chunk of candidates), no barrier.
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
#include "topk_mfma_device.h"

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

// The head of this form (topk_device.h); topk_mfma_device.h's two streams read its fields
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
template <int KT_, int MT, int QT_>
struct RfmWave {
    typedef RfmHead Head;
    static constexpr int KT = KT_, QT = QT_;
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

// the wave of class <KT, MT>
template <int KT, int MT>
using RfmClass = RfmWave<KT, MT, rfm_qt(KT, MT)>;

// KT by D (2, 4, 10, 20 MFMAs over the input width), MT by M (1, 2, 3, 5 tiles of 16 rows): sixteen of each kernel.
// TransNet(++) at latent sizes 6 / 10 / 16 / 32 / 64 lands on <2 | 4, 1>, <4 | 10, 2>, <4 | 10, 2>, <10, 3>, <20, 5>.
inline int rfm_kt(int D) { return D <= 8 ? 2 : D <= 16 ? 4 : D <= 40 ? 10 : 20; }
inline int rfm_mt(int M) { return M <= 16 ? 1 : M <= 32 ? 2 : M <= 48 ? 3 : 5; }
// the queries (pairs) per wave of the instantiation that serves (D, M)
inline int rfm_tile(int D, int M) { return rfm_qt(rfm_kt(D), rfm_mt(M)); }

#define RFM_DISPATCH(FN, D, M, ...)                                                    \
    do {                                                                               \
        switch (rfm_kt(D) * 8 + rfm_mt(M)) {                                           \
        case 2 * 8 + 1: return FN<RfmClass<2, 1>>(__VA_ARGS__);                        \
        case 2 * 8 + 2: return FN<RfmClass<2, 2>>(__VA_ARGS__);                        \
        case 2 * 8 + 3: return FN<RfmClass<2, 3>>(__VA_ARGS__);                        \
        case 2 * 8 + 5: return FN<RfmClass<2, 5>>(__VA_ARGS__);                        \
        case 4 * 8 + 1: return FN<RfmClass<4, 1>>(__VA_ARGS__);                        \
        case 4 * 8 + 2: return FN<RfmClass<4, 2>>(__VA_ARGS__);                        \
        case 4 * 8 + 3: return FN<RfmClass<4, 3>>(__VA_ARGS__);                        \
        case 4 * 8 + 5: return FN<RfmClass<4, 5>>(__VA_ARGS__);                        \
        case 10 * 8 + 1: return FN<RfmClass<10, 1>>(__VA_ARGS__);                      \
        case 10 * 8 + 2: return FN<RfmClass<10, 2>>(__VA_ARGS__);                      \
        case 10 * 8 + 3: return FN<RfmClass<10, 3>>(__VA_ARGS__);                      \
        case 10 * 8 + 5: return FN<RfmClass<10, 5>>(__VA_ARGS__);                      \
        case 20 * 8 + 1: return FN<RfmClass<20, 1>>(__VA_ARGS__);                      \
        case 20 * 8 + 2: return FN<RfmClass<20, 2>>(__VA_ARGS__);                      \
        case 20 * 8 + 3: return FN<RfmClass<20, 3>>(__VA_ARGS__);                      \
        default: return FN<RfmClass<20, 5>>(__VA_ARGS__);                              \
        }                                                                              \
    } while (0)

int dispatch_rfm_scan(const MfmaScanArgs<RfmHead> &a, hipStream_t st) {
    RFM_DISPATCH(launch_mfma_scan, a.h.D, a.h.M, "rfm_scan_kernel", a, st);
}
int dispatch_rfm_rank(const MfmaRankArgs<RfmHead> &a, int64_t parts, hipStream_t st) {
    RFM_DISPATCH(launch_mfma_rank, a.h.D, a.h.M, "rank_rfm_scan_kernel", a, parts, st);
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
    const RfmHead h = rfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, l, H, P, M);
    return mfma_topk_call("topk_rfm", h, RFM_CHUNK_QT, rfm_tile(h.D, M), dispatch_rfm_scan, n_q, excl_off, excl_ids, K,
                          chunk, ws, ws_bytes, out_ids, out_scores, stream);
}

extern "C" int r4r_pair_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                            const float *c_bias, const float *W, const float *b, const float *s, const float *l, int H, int P,
                            int M, const int64_t *q_idx, const int64_t *c_idx, int64_t n, float *out, void *stream) {
    const RfmHead h = rfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, l, H, P, M);
    return mfma_pair_call("pair_rfm", h, n_q, q_idx, c_idx, n, out, stream);
}

extern "C" int r4r_rank_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                            const float *c_bias, const float *W, const float *b, const float *s, const float *l, int H, int P,
                            int M, const int64_t *q_idx, const int64_t *t_idx, int64_t n_p, const int64_t *excl_off,
                            const int64_t *excl_ids, int64_t chunk, int64_t *out_rank, float *out_score, void *stream) {
    const RfmHead h = rfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, l, H, P, M);
    return mfma_rank_call("rank_rfm", h, RFM_CHUNK_QT, rfm_tile(h.D, M), dispatch_rfm_rank, n_q, q_idx, t_idx, n_p, excl_off,
                          excl_ids, chunk, out_rank, out_score, stream);
}

// Slates (slate_device.h): the K best of, and the place of a target among, per-query candidate lists
extern "C" int r4r_slate_topk_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c,
                                  int64_t c_stride, const float *c_bias, const float *W, const float *b, const float *s,
                                  const float *l, int H, int P, int M, const int64_t *q_idx, const int64_t *slate_off,
                                  const int64_t *slate_ids, int64_t n_s, int64_t max_len, const int64_t *excl_off,
                                  const int64_t *excl_ids, int K, void *ws, size_t ws_bytes, int64_t *out_ids,
                                  float *out_scores, void *stream) {
    const RfmHead h = rfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, l, H, P, M);
    return mfma_slate_topk_call("slate_topk_rfm", h, n_q, q_idx, slate_off, slate_ids, n_s, max_len, excl_off, excl_ids,
                                K, ws, ws_bytes, out_ids, out_scores, stream);
}

extern "C" int r4r_slate_rank_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c,
                                  int64_t c_stride, const float *c_bias, const float *W, const float *b, const float *s,
                                  const float *l, int H, int P, int M, const int64_t *q_idx, const int64_t *t_idx,
                                  const int64_t *slate_off, const int64_t *slate_ids, int64_t n_p, int64_t max_len,
                                  const int64_t *excl_off, const int64_t *excl_ids, int64_t *out_rank, float *out_score,
                                  void *stream) {
    const RfmHead h = rfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, l, H, P, M);
    return mfma_slate_rank_call("slate_rank_rfm", h, n_q, q_idx, t_idx, slate_off, slate_ids, n_p, max_len, excl_off,
                                excl_ids, out_rank, out_score, stream);
}

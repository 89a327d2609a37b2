// Catalogue top-K and ranks over a product-MLP head: r4r_topk_hmlp / r4r_pair_hmlp / r4r_rank_hmlp (include/r4r.h,
// "Catalogue recommendation: product-MLP heads").
//
//   x_m = q[u][m] * c[i][m]            y_j = fmaf(W[j][m], x_m, y_j)   m ascending       z_j = fmaxf(y_j + b[j], 0)
//   h_g = fmaf(w[j], z_j, h_g)   over the j with ((j >> 2) & 3) == g, ascending
//   score(u, i) = ((((h_0 + h_1) + (h_2 + h_3)) + c_bias[i]) + q_bias[u])
//
// The ReLU sits behind an H x D matrix product per pair: matrix-core work, but not topk.hip's shape.  Here the A operand
// of v_mfma_f32_16x16x4_f32 is the head's matrix W, shared by every pair, and the B operand is formed in registers:
// rows = hidden units, columns = 16 candidates, k = the input width.
// Launch 1, mfma_scan_kernel<HmlpWave> (topk_mfma_device.h has the stream): one WAVE per workgroup = (tile of HMLP_QT
// queries) x (chunk of candidates), no barrier.
//   A  lane l supplies W[16 ht + (l & 15)][4 t + (l >> 4)] for MFMA (ht, t): loaded once, kept for the whole chunk.
//   B  lane l loads c[slab + (l & 15)][4 t + (l >> 4)] (one dword per lane and t, as topk.hip does and for its reason) and
//      multiplies it by its query's q[u][4 t + (l >> 4)]: x, one v_mul_f32 per B fragment.  The tile's queries reuse the
//      slab's c registers; the next slab's loads are issued before this slab's MFMAs.
//   C  lane l holds y of hidden units 16 ht + 4 (l >> 4) + r, r = 0 .. 3, for candidate l & 15: the epilogue adds b, takes
//      fmaxf and runs the h_g chain of ITS lane group g = l >> 4 over (ht, r); two cross-lane adds (xor 16, xor 32: both
//      orders of either add give the same bits) finish the sum, then the two biases.
// Scores are never written: each is compared with its query's K-th best, survivors go through topk_device.h's
// list_insert, the partial lists have r4r_topk_dot's workspace layout and topk.hip's merge kernel finishes (skipped for a
// single chunk).  r4r_rank_hmlp: the same stream over a tile of PAIRS with counters in place of lists.
// topk_device.h's scalar kernels (pairs, rank targets, the exclusion correction) over this file's HmlpHead compute
// hmlp_pair_score: the chain above written out.  v_mfma_f32_16x16x4_f32 is bitwise that chain over m (topk.hip), zero
// rows of W give z = 0 and w = 0 adds nothing, so a score's bits depend on its own pair only.
// This file has the chain, the head and the wave; the two streams and the host sequence of a call are
// topk_mfma_device.h's, shared with topk_rfm.hip; the scalar kernels, the chunk rule, the argument checks and the plan
// of a call are topk_device.h's, shared with every form.
#include <math.h>

#include "common.h"
#include "topk_device.h"
#include "topk_mfma_device.h"

namespace r4r {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HMLP_MAX_D = 64;
constexpr int HMLP_MAX_H = 64;
constexpr int HMLP_QT = 4;         // queries (pairs, for the rank) per wave

// the scalar chain of one pair: q, c point at the pair's rows.  (g is a compile-time index: h stays in registers.)
__device__ __forceinline__ float hmlp_pair_score(const float *q, const float *c, const float *W, const float *b, const float *w,
                                                 int D, int H, float cb, float qb) {
    float h[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < H; j0 += 16) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 4 * g + r;
                if (j >= H) break;
                const float *Wj = W + (size_t)j * D;
                float y = 0.f;
                for (int m = 0; m < D; ++m) {
                    const float x = q[m] * c[m];
                    y = __builtin_fmaf(Wj[m], x, y);
                }
                const float z = __builtin_fmaxf(y + (b != nullptr ? b[j] : 0.f), 0.f);
                h[g] = __builtin_fmaf(w[j], z, h[g]);
            }
        }
    }
    return (((h[0] + h[1]) + (h[2] + h[3])) + cb) + qb;
}

// The head of this form (topk_device.h); topk_mfma_device.h's two streams read its fields
struct HmlpHead {
    const float *q, *q_bias, *c, *c_bias, *W, *b, *w;
    int64_t n_c, c_stride;
    int D, H;

    __device__ __forceinline__ float q_bias_of(int64_t u) const { return q_bias ? q_bias[u] : 0.f; }
    __device__ __forceinline__ float score(int64_t u, int64_t i, float qb) const {
        return hmlp_pair_score(q + u * D, c + i * c_stride, W, b, w, D, H, c_bias ? c_bias[i] : 0.f, qb);
    }
    __device__ __forceinline__ float score(int64_t u, int64_t i) const { return score(u, i, q_bias_of(u)); }

    static constexpr const char *width_name = "D";
    int width() const { return D; }
    int ranges(const char *fn) const {
        R4R_REQUIRE(D >= 0 && D <= HMLP_MAX_D, "%s: D = %d outside 0 .. %d", fn, D, HMLP_MAX_D);
        R4R_REQUIRE(H >= 0 && H <= HMLP_MAX_H, "%s: H = %d outside 0 .. %d", fn, H, HMLP_MAX_H);
        return R4R_OK;
    }
    int weights(const char *fn) const {
        R4R_REQUIRE(H == 0 || (w != nullptr && W != nullptr), "%s: null w or W with H > 0", fn);
        return R4R_OK;
    }
};

// What a wave keeps for its whole chunk: the head (A fragments; b and w in the accumulator layout) and the column of
// each B fragment.  KT: MFMAs over the input width (D <= 4 KT), HT: 16-row tiles of hidden units (H <= 16 HT).
template <int KT_, int HT>
struct HmlpWave {
    typedef HmlpHead Head;
    static constexpr int KT = KT_, QT = HMLP_QT;
    float wf[HT][KT];          // W[16 ht + row][4 t + kq]; zero beyond H and beyond D
    float bj[HT][4], wj[HT][4];// b / w of hidden unit 16 ht + 4 kq + r; zero beyond H (and for a NULL b)
    int jo[KT];                // the column lane (., kq) reads for MFMA t, clamped into the row
    int row, kq;

    __device__ __forceinline__ void init(const HmlpHead &a, int lane) {
        row = lane & 15;
        kq = lane >> 4;
        const int D = a.D, H = a.H;
#pragma unroll
        for (int t = 0; t < KT; ++t) jo[t] = (4 * t + kq < D) ? 4 * t + kq : (D > 0 ? D - 1 : 0);
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) {
            const int j = 16 * ht + row;
            const int jc = j < H ? j : (H > 0 ? H - 1 : 0);
#pragma unroll
            for (int t = 0; t < KT; ++t) wf[ht][t] = 0.f;
            if (D > 0 && H > 0) {
#pragma unroll
                for (int t = 0; t < KT; ++t) wf[ht][t] = a.W[(size_t)jc * D + jo[t]];
            }
#pragma unroll
            for (int t = 0; t < KT; ++t) wf[ht][t] = (j < H && 4 * t + kq < D) ? wf[ht][t] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = 16 * ht + 4 * kq + r;
                const int ec = e < H ? e : (H > 0 ? H - 1 : 0);
                float bv = 0.f, wv = 0.f;
                if (H > 0) {
                    wv = a.w[ec];
                    if (a.b != nullptr) bv = a.b[ec];
                }
                bj[ht][r] = e < H ? bv : 0.f;
                wj[ht][r] = e < H ? wv : 0.f;
            }
        }
    }

    // the query row `src` as B-fragment multipliers: q[.][4 t + kq], zero beyond D (and for a row that does not exist)
    __device__ __forceinline__ void query(const HmlpHead &a, const float *src, bool exists, float (&qf)[KT]) const {
#pragma unroll
        for (int t = 0; t < KT; ++t) qf[t] = 0.f;
        if (a.D > 0) {
#pragma unroll
            for (int t = 0; t < KT; ++t) qf[t] = src[jo[t]];
        }
#pragma unroll
        for (int t = 0; t < KT; ++t) qf[t] = (exists && 4 * t + kq < a.D) ? qf[t] : 0.f;
    }

    // The slab's c registers against HMLP_QT queries -> sv[s], the score of candidate `row` for query s (the same in all
    // four lanes of a candidate), without the query's bias.
    __device__ __forceinline__ void scores(const float (&bf)[KT], const float (&qf)[HMLP_QT][KT], float cb,
                                           float (&sv)[HMLP_QT]) const {
        f32x4 acc[HMLP_QT][HT];
#pragma unroll
        for (int s = 0; s < HMLP_QT; ++s)
#pragma unroll
            for (int ht = 0; ht < HT; ++ht) acc[s][ht] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // every accumulator sees t ascending; the HMLP_QT * HT chains are independent and interleave in the matrix pipe
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int s = 0; s < HMLP_QT; ++s) {
                const float x = bf[t] * qf[s][t];
#pragma unroll
                for (int ht = 0; ht < HT; ++ht)
                    acc[s][ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[ht][t], x, acc[s][ht], 0, 0, 0);
            }
#pragma unroll
        for (int s = 0; s < HMLP_QT; ++s) {
            float h = 0.f;                                     // h_g of this lane's group g = kq
#pragma unroll
            for (int ht = 0; ht < HT; ++ht)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    h = __builtin_fmaf(wj[ht][r], __builtin_fmaxf(acc[s][ht][r] + bj[ht][r], 0.f), h);
            h = h + __shfl_xor(h, 16);                         // h_0 + h_1 | h_2 + h_3
            h = h + __shfl_xor(h, 32);                         // (h_0 + h_1) + (h_2 + h_3)
            sv[s] = h + cb;
        }
    }
};

// KT by D (2, 4, 8, 16 MFMAs over the input width), HT by H (1 .. 4 tiles of 16 hidden units)
#define HMLP_DISPATCH(FN, D, H, ...)                                                   \
    do {                                                                               \
        const int kt_ = (D) <= 8 ? 2 : (D) <= 16 ? 4 : (D) <= 32 ? 8 : 16;             \
        const int ht_ = (H) <= 16 ? 1 : (H) <= 32 ? 2 : (H) <= 48 ? 3 : 4;             \
        switch (kt_ * 8 + ht_) {                                                       \
        case 2 * 8 + 1: return FN<HmlpWave<2, 1>>(__VA_ARGS__);                        \
        case 2 * 8 + 2: return FN<HmlpWave<2, 2>>(__VA_ARGS__);                        \
        case 2 * 8 + 3: return FN<HmlpWave<2, 3>>(__VA_ARGS__);                        \
        case 2 * 8 + 4: return FN<HmlpWave<2, 4>>(__VA_ARGS__);                        \
        case 4 * 8 + 1: return FN<HmlpWave<4, 1>>(__VA_ARGS__);                        \
        case 4 * 8 + 2: return FN<HmlpWave<4, 2>>(__VA_ARGS__);                        \
        case 4 * 8 + 3: return FN<HmlpWave<4, 3>>(__VA_ARGS__);                        \
        case 4 * 8 + 4: return FN<HmlpWave<4, 4>>(__VA_ARGS__);                        \
        case 8 * 8 + 1: return FN<HmlpWave<8, 1>>(__VA_ARGS__);                        \
        case 8 * 8 + 2: return FN<HmlpWave<8, 2>>(__VA_ARGS__);                        \
        case 8 * 8 + 3: return FN<HmlpWave<8, 3>>(__VA_ARGS__);                        \
        case 8 * 8 + 4: return FN<HmlpWave<8, 4>>(__VA_ARGS__);                        \
        case 16 * 8 + 1: return FN<HmlpWave<16, 1>>(__VA_ARGS__);                      \
        case 16 * 8 + 2: return FN<HmlpWave<16, 2>>(__VA_ARGS__);                      \
        case 16 * 8 + 3: return FN<HmlpWave<16, 3>>(__VA_ARGS__);                      \
        default: return FN<HmlpWave<16, 4>>(__VA_ARGS__);                              \
        }                                                                              \
    } while (0)

int dispatch_hmlp_scan(const MfmaScanArgs<HmlpHead> &a, hipStream_t st) {
    HMLP_DISPATCH(launch_mfma_scan, a.h.D, a.h.H, "hmlp_scan_kernel", a, st);
}
int dispatch_hmlp_rank(const MfmaRankArgs<HmlpHead> &a, int64_t parts, hipStream_t st) {
    HMLP_DISPATCH(launch_mfma_rank, a.h.D, a.h.H, "rank_hmlp_scan_kernel", a, parts, st);
}

inline HmlpHead hmlp_head(const float *q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                          const float *c_bias, const float *W, const float *b, const float *w, int D, int H) {
    HmlpHead h;
    h.q = q; h.q_bias = q_bias; h.c = c; h.c_bias = c_bias; h.W = W; h.b = b; h.w = w;
    h.n_c = n_c; h.c_stride = c_stride; h.D = D; h.H = H;
    return h;
}

}  // namespace
}  // namespace r4r

using namespace r4r;

extern "C" size_t r4r_topk_hmlp_ws_bytes(int64_t n_q, int64_t n_c, int K, int64_t chunk) {
    return lists_ws_bytes(n_q, n_c, K, chunk, HMLP_QT);
}

extern "C" int r4r_topk_hmlp(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                             const float *c_bias, const float *W, const float *b, const float *w, int D, int H,
                             const int64_t *excl_off, const int64_t *excl_ids, int K, int64_t chunk, void *ws, size_t ws_bytes,
                             int64_t *out_ids, float *out_scores, void *stream) {
    const HmlpHead h = hmlp_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, w, D, H);
    return mfma_topk_call("topk_hmlp", h, HMLP_QT, HMLP_QT, dispatch_hmlp_scan, n_q, excl_off, excl_ids, K, chunk, ws,
                          ws_bytes, out_ids, out_scores, stream);
}

extern "C" int r4r_pair_hmlp(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                             const float *c_bias, const float *W, const float *b, const float *w, int D, int H,
                             const int64_t *q_idx, const int64_t *c_idx, int64_t n, float *out, void *stream) {
    const HmlpHead h = hmlp_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, w, D, H);
    return mfma_pair_call("pair_hmlp", h, n_q, q_idx, c_idx, n, out, stream);
}

extern "C" int r4r_rank_hmlp(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                             const float *c_bias, const float *W, const float *b, const float *w, int D, int H,
                             const int64_t *q_idx, const int64_t *t_idx, int64_t n_p, const int64_t *excl_off,
                             const int64_t *excl_ids, int64_t chunk, int64_t *out_rank, float *out_score, void *stream) {
    const HmlpHead h = hmlp_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, w, D, H);
    return mfma_rank_call("rank_hmlp", h, HMLP_QT, HMLP_QT, dispatch_hmlp_rank, n_q, q_idx, t_idx, n_p, excl_off, excl_ids,
                          chunk, out_rank, out_score, stream);
}

// Slates (slate_device.h): the K best of, and the place of a target among, per-query candidate lists
extern "C" int r4r_slate_topk_hmlp(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c,
                                   int64_t c_stride, const float *c_bias, const float *W, const float *b,
                                   const float *w, int D, int H, const int64_t *q_idx, const int64_t *slate_off,
                                   const int64_t *slate_ids, int64_t n_s, int64_t max_len, const int64_t *excl_off,
                                   const int64_t *excl_ids, int K, void *ws, size_t ws_bytes, int64_t *out_ids,
                                   float *out_scores, void *stream) {
    const HmlpHead h = hmlp_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, w, D, H);
    return mfma_slate_topk_call("slate_topk_hmlp", h, n_q, q_idx, slate_off, slate_ids, n_s, max_len, excl_off,
                                excl_ids, K, ws, ws_bytes, out_ids, out_scores, stream);
}

extern "C" int r4r_slate_rank_hmlp(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c,
                                   int64_t c_stride, const float *c_bias, const float *W, const float *b,
                                   const float *w, int D, int H, const int64_t *q_idx, const int64_t *t_idx,
                                   const int64_t *slate_off, const int64_t *slate_ids, int64_t n_p, int64_t max_len,
                                   const int64_t *excl_off, const int64_t *excl_ids, int64_t *out_rank,
                                   float *out_score, void *stream) {
    const HmlpHead h = hmlp_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, w, D, H);
    return mfma_slate_rank_call("slate_rank_hmlp", h, n_q, q_idx, t_idx, slate_off, slate_ids, n_p, max_len, excl_off,
                                excl_ids, out_rank, out_score, stream);
}

// The variant pass of NARRE's what-if scores and counterfactual search: what narre_whatif.hip and narre_search.hip share.
// A pair's rating under two masks of removed slots is a re-selection of slots, a softmax over R logits, a pooled vector per
// side and the L x L head (NARRE.attention, pytorch_models/NARRE.py:53-64; the head of NARRE.py:38-46, 115-124; a removal
// is the loader's `skip`, data.py:144-172, 275-279).  r4r_narre_search promises r4r_narre_whatif's bits for the same pair
// under the same masks (include/r4r.h); the arithmetic behind that promise is here, once:
//
//   variant_pooled  one side under a mask: lane s ranks slot s among the clear bits below it (one popcount) and, below R,
//                   scatters itself to its place of the selected list; the places beyond hold the pad row.  Lane k then
//                   holds the k-th selected logit: wave_max, expf, wave_sum, one division -> a'_k; lane l chains
//                   o'_l = fmaf(a'_k, z'_k[l], o'_l) over k ascending out of the staged rows (row stride L: consecutive
//                   lanes, conflict free);
//   variant_head    the 16 rows of the x tile (row stride 66 floats: the B-fragment reads are conflict free in both
//                   32-lane halves) are the columns of v_mfma_f32_16x16x4_f32 with W1 as A in topk_hmlp.hip's fragment
//                   layout, t ascending; ReLU, w and two __shfl_xor adds in the epilogue.  A column depends on that
//                   column's B values only.
// Host side: the slice size, the argument checks both entry points share, the waves that fit into LDS, the dispatch on
// the class of L.  Each kernel keeps its own argument struct, staging and fragment loads: measured, a
// shared copy of those moved their scalar spills or their speed.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"

namespace r4r {

typedef float nv_f32x4 __attribute__((ext_vector_type(4)));

constexpr int NV_MAXS = 64, NV_MAXL = 64;
constexpr int NV_GROUP = 16;           // variants per wave pass: the columns of one MFMA tile
constexpr int NV_XS = 66;              // floats per row of the x tile: bank (mod 32) = 2 column + k quarter
constexpr int NV_LG = NV_MAXS + 4;     // floats per side's staged logits: S + the pad slot, rounded to 16 bytes
constexpr int NV_MAX_WAVES = 4;        // waves per workgroup, fewer where their LDS slices would pass 64 KiB
constexpr int NV_LDS_BYTES = 64 * 1024;

// Floats of one wave's slice of dynamic LDS: x tile | sel | user logits | item logits | user rows | item rows.
inline size_t variant_slice_floats(int S_u, int S_i, int L) {
    const size_t n = (size_t)NV_GROUP * NV_XS + WAVE + 2 * NV_LG + (size_t)(S_u + 1 + S_i + 1) * L;
    return (n + 3) & ~(size_t)3;
}

// One side under `mask`: the selected list, its softmax and the pooled vector o' (lane l; 0 past L).
// zs: the side's staged rows [S + 1, L] (row S = z_pad), lgs: its staged logits [S + 1], sel: 64 ints of the wave.
__device__ __forceinline__ float variant_pooled(const float *zs, const float *lgs, int *sel, uint64_t mask, int S, int R,
                                                int L, int lane) {
    const uint64_t all = S >= 64 ? ~0ull : ((1ull << S) - 1ull);
    const uint64_t keep = ~mask & all;                         // bits at positions >= S are ignored
    const int left = __builtin_popcountll(keep);
    const int nsel = left < R ? left : R;
    const int rank = __builtin_popcountll(keep & ((1ull << lane) - 1ull));
    wave_lds_fence();                                          // the reads of the list before are done
    if (((keep >> lane) & 1ull) && rank < R) sel[rank] = lane;
    if (lane >= nsel && lane < R) sel[lane] = S;               // the pad slot
    wave_lds_fence();
    const int sk = lane < R ? sel[lane] : S;                   // lane k: the k-th selected slot
    const float lg = lane < R ? lgs[sk] : -INFINITY;
    const float m = wave_max(lg);
    const float e = lane < R ? expf(lg - m) : 0.f;
    const float den = wave_sum(e);
    const float w = e / den;                                   // lane k: a'_k; 0 in the lanes past R
    float o = 0.f;
    const int l = lane < L ? lane : 0;
    for (int k = 0; k < R; ++k) {
        const int s = __builtin_amdgcn_readlane(sk, k);
        o = fmaf(lane_value(w, k), zs[s * L + l], o);
    }
    return lane < L ? o : 0.f;
}

// The head over the 16 rows of the x tile -> lanes 0 .. 15: the head of tile row `lane` (before the biases).
// LT: the class of L (L <= 16 LT); wf, bj, wj: variant_head_load's fragments; row = lane & 15, kq = lane >> 4.
template <int LT>
__device__ __forceinline__ float variant_head(const float *xs, const float (&wf)[LT][4 * LT], const float (&bj)[LT][4],
                                              const float (&wj)[LT][4], int row, int kq) {
    constexpr int KT = 4 * LT, HT = LT;
    nv_f32x4 acc[HT];
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) acc[ht] = (nv_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KT; ++t) {                             // every accumulator sees t ascending
        const float xb = xs[row * NV_XS + 4 * t + kq];
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) acc[ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[ht][t], xb, acc[ht], 0, 0, 0);
    }
    float h = 0.f;                                             // h_g of this lane's group g = kq
#pragma unroll
    for (int ht = 0; ht < HT; ++ht)
#pragma unroll
        for (int r = 0; r < 4; ++r) h = __builtin_fmaf(wj[ht][r], __builtin_fmaxf(acc[ht][r] + bj[ht][r], 0.f), h);
    h = h + __shfl_xor(h, 16);                                 // h_0 + h_1 | h_2 + h_3
    h = h + __shfl_xor(h, 32);                                 // (h_0 + h_1) + (h_2 + h_3)
    return h;
}

// ---------------------------------------------------------------- host side

// What r4r_narre_whatif and r4r_narre_search (`fn`) ask of the arguments they share: R4R_OK or R4R_ERR_ARG with the
// error set.  A call without pairs has its sizes checked, not its pointers.
inline int variant_require(const char *fn, const float *z_u, const float *logit_u, const float *z_pad_u, int64_t n_u,
                           int S_u, int R_u, const float *z_i, const float *logit_i, const float *z_pad_i, int64_t n_i,
                           int S_i, int R_i, const int64_t *u_idx, const int64_t *i_idx, int64_t n_p, const float *W1,
                           const float *b1, const float *w, int L) {
    R4R_REQUIRE(S_u >= 1 && S_u <= NV_MAXS, "%s: S_u=%d slots outside 1..%d", fn, S_u, NV_MAXS);
    R4R_REQUIRE(S_i >= 1 && S_i <= NV_MAXS, "%s: S_i=%d slots outside 1..%d", fn, S_i, NV_MAXS);
    R4R_REQUIRE(R_u >= 1 && R_u <= S_u, "%s: R_u=%d attended slots outside 1..S_u=%d", fn, R_u, S_u);
    R4R_REQUIRE(R_i >= 1 && R_i <= S_i, "%s: R_i=%d attended slots outside 1..S_i=%d", fn, R_i, S_i);
    R4R_REQUIRE(L >= 1 && L <= NV_MAXL, "%s: L=%d latent units outside 1..%d", fn, L, NV_MAXL);
    R4R_REQUIRE(n_u >= 0 && n_i >= 0, "%s: n_u=%lld / n_i=%lld negative", fn, (long long)n_u, (long long)n_i);
    if (n_p == 0) return R4R_OK;
    R4R_REQUIRE(z_u && logit_u && z_pad_u, "%s: null pointer among z_u, logit_u, z_pad_u", fn);
    R4R_REQUIRE(z_i && logit_i && z_pad_i, "%s: null pointer among z_i, logit_i, z_pad_i", fn);
    R4R_REQUIRE(u_idx && i_idx, "%s: null pointer among u_idx, i_idx", fn);
    R4R_REQUIRE(W1 && b1 && w, "%s: null pointer among W1, b1, w", fn);
    R4R_REQUIRE(n_u >= 1 && n_i >= 1, "%s: n_p=%lld pairs over n_u=%lld / n_i=%lld rows", fn, (long long)n_p,
                (long long)n_u, (long long)n_i);
    return R4R_OK;
}

// The waves of a workgroup whose slices of `slice` floats fit into LDS.
inline int variant_waves(size_t slice) {
    int waves = NV_MAX_WAVES;
    while (waves > 1 && waves * slice * sizeof(float) > (size_t)NV_LDS_BYTES) waves >>= 1;
    return waves;
}

// launch(std::integral_constant<int, LT>) with LT the class of L.
template <class Launch>
inline void variant_dispatch(int L, Launch launch) {
    if (L <= 16)
        launch(std::integral_constant<int, 1>());
    else if (L <= 32)
        launch(std::integral_constant<int, 2>());
    else if (L <= 48)
        launch(std::integral_constant<int, 3>());
    else
        launch(std::integral_constant<int, 4>());
}

}  // namespace r4r

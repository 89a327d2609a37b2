// NARRE what-if scores for gfx950 (include/r4r.h, "NARRE what-if scores"): a pair's eval-mode rating with chosen reviews
// of either owner REMOVED, exactly as the loader removes a review (`skip`, data.py:144-172, 275-279: slot r holds the
// r-th REMAINING review, the next review beyond R slides in, padding fills the tail).  A review enters NARRE's score only
// through its own latent z_r and its own attention logit, so nothing of a tower runs again: an owner pass
// (r4r_narre_logits) returns the PRE-softmax logit of every slot once per owner, and a variant pass (r4r_narre_whatif)
// re-selects, re-normalises, pools and scores every (pair, variant).
//
// Reference behaviour restated: NARRE.attention, pytorch_models/NARRE.py:53-64, in eval mode, the scorer of
// NARRE.py:24-36 and the head of NARRE.py:38-46, 115-124 (dropout is the identity in eval mode).
//
// Owner pass: narre_explain.hip's kernel shape -- one WAVE per owner, LOGIT_WAVES waves share one LDS image of W0 -- and
// its logits over S <= 64 slots: the same functions of csrc/narre_attn_device.h, so a slot's logit has the bits that feed
// r4r_narre_explain's softmax.
// Variant pass: one WAVE per (pair, group of 16 variants), grid-strided; the waves of a workgroup are independent.
//   1. the wave stages the pair's two z blocks [S, L] and logits [S] in its own LDS slice, the pad slot (z_pad,
//      logit_pad) as row S of each;
//   2. per variant and side, csrc/narre_variant_device.h's variant_pooled (the counterfactual search calls the same
//      function): the selected list of the mask, its softmax, the pooled vector o'; a side whose mask repeats keeps it;
//   3. x = (o'_u + own_u) o (o'_i + own_i) of the variant goes to row (variant mod 16) of an LDS tile (row stride 66);
//   4. the 16 variants are the columns of v_mfma_f32_16x16x4_f32: A = W1 in topk_hmlp.hip's fragment layout, loaded once
//      per wave, B = x read from the tile; ReLU, w and the biases in the epilogue -- variant_head's sequence, inline here
//      as before (as a call it changed this kernel's code at L <= 32).
// A column of the MFMA depends on that column's B values only, so a variant's bits depend on its own pair's inputs, its
// ordered selected list and its pad count: not on V, its column, n_p, the grid or the other variants.
// Both kernels read their argument struct through kernel_args<>() (common.h).
#include "common.h"
#include "narre_attn_device.h"
#include "narre_variant_device.h"

namespace r4r {

constexpr int WI_MAXS = 64, WI_MAXL = 64;
constexpr int LOGIT_WAVES = 8;         // waves (= owners in flight) per workgroup, sharing one image of W0
constexpr int LOGIT_SLOTS = 5;         // slots per staged group: narre_explain.hip's EX_SLOTS (the bits do not depend on it)
constexpr int LOGIT_MAX_BLOCKS = 1024; // beyond, a workgroup's waves loop over owners
constexpr int WI_MAX_BLOCKS = 8192;    // beyond, a workgroup's waves loop over (pair, group)

struct LogitArgs {
    const float *z;
    const int64_t *nb;
    const float *other_table;
    int64_t other_rows;
    const float *W0, *b0, *w3, *b3;
    float *logit;
    int64_t N;
    int S, L;
};

struct WhatifSide {                    // one side of a pair
    const float *z, *logit, *own, *z_pad;
    const int64_t *drop;
    float logit_pad;
    int S, R;
};

struct WhatifArgs {
    WhatifSide user, item;
    const int64_t *u_idx, *i_idx;
    int64_t n_p;
    int V;
    const float *q_bias, *c_bias, *W1, *b1, *w;
    int L;
    int slice;                         // floats of one wave's LDS slice
    float *out_score;
};

// LMAX: the class of L (L <= LMAX) -- it fixes the LDS strides, nothing of the arithmetic.
template <int LMAX>
__global__ __launch_bounds__(LOGIT_WAVES *WAVE) void narre_logits_kernel(const LogitArgs) {
    const LogitArgs &a = kernel_args<LogitArgs>();             // each field an s_load next to its use (common.h)
    __shared__ __attribute__((aligned(16))) float w0s[LMAX * ATTN_WS<LMAX>];
    __shared__ __attribute__((aligned(16))) float cats[LOGIT_WAVES][LOGIT_SLOTS * ATTN_CS<LMAX>];
    const int S = a.S, L = a.L;
    attn_stage_w0<LMAX>(w0s, a.W0, L, LOGIT_WAVES * WAVE);
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    float *cat = cats[wave];
    const AttnLane ln = attn_lane<LMAX>(w0s, a.b0, a.w3, a.b3, L, lane);
    const int64_t N = a.N, other_rows = a.other_rows;
    const float *other_table = a.other_table;
    for (int64_t n = (int64_t)blockIdx.x * LOGIT_WAVES + wave; n < N; n += (int64_t)gridDim.x * LOGIT_WAVES) {
        const float *zn = a.z + n * S * L;
        const int64_t *nbn = a.nb + n * S;
        float sc = 0.f;                                        // lane s: the logit of slot s
        for (int r0 = 0; r0 < S; r0 += LOGIT_SLOTS)
            attn_group_logits<LMAX, LOGIT_SLOTS>(cat, zn, nbn, other_table, other_rows, r0, S, L, ln, lane, sc);
        if (lane < S) a.logit[n * S + lane] = sc;
    }
}

// LT: the class of L (L <= 16 LT): 4 LT MFMAs over the input width, LT 16-row tiles of hidden units.
template <int LT>
__global__ __launch_bounds__(NV_MAX_WAVES *WAVE) void narre_whatif_kernel(const WhatifArgs) {
    const WhatifArgs &a = kernel_args<WhatifArgs>();           // each field an s_load next to its use (common.h)
    constexpr int KT = 4 * LT, HT = LT;
    extern __shared__ __attribute__((aligned(16))) float wi_lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int waves = __builtin_amdgcn_readfirstlane(blockDim.x / WAVE);
    const int L = a.L, V = a.V;
    const int Su = a.user.S, Si = a.item.S, Ru = a.user.R, Ri = a.item.R;
    // the wave's slice: x tile | sel | user logits | item logits | user rows | item rows
    float *xs = wi_lds + (size_t)wave * a.slice;
    int *sel = reinterpret_cast<int *>(xs + NV_GROUP * NV_XS);
    float *lgu = xs + NV_GROUP * NV_XS + WAVE;
    float *lgi = lgu + (NV_MAXS + 4);
    float *zu = lgi + (NV_MAXS + 4);
    float *zi = zu + (Su + 1) * L;
    const int row = lane & 15, kq = lane >> 4;
    // A fragments of W1 and the epilogue's b1 / w in the accumulator layout (topk_hmlp.hip's HmlpWave::init); zero
    // beyond L, so that the tile's pad columns and the rows past L count for nothing
    float wf[HT][KT], bj[HT][4], wj[HT][4];
    {
        const float *W1 = a.W1, *b1 = a.b1, *wv = a.w;
        // every load first, from clamped addresses, the masks afterwards: the loads are issued back to back
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) {
            const int j = 16 * ht + row;
            const float *Wj = W1 + (size_t)(j < L ? j : L - 1) * L;
#pragma unroll
            for (int t = 0; t < KT; ++t) wf[ht][t] = Wj[4 * t + kq < L ? 4 * t + kq : L - 1];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = 16 * ht + 4 * kq + r;
                bj[ht][r] = b1[e < L ? e : L - 1];
                wj[ht][r] = wv[e < L ? e : L - 1];
            }
        }
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) {
#pragma unroll
            for (int t = 0; t < KT; ++t) wf[ht][t] = (16 * ht + row < L && 4 * t + kq < L) ? wf[ht][t] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = 16 * ht + 4 * kq + r < L;
                bj[ht][r] = in ? bj[ht][r] : 0.f;
                wj[ht][r] = in ? wj[ht][r] : 0.f;
            }
        }
    }
    const int groups = (V + NV_GROUP - 1) / NV_GROUP;
    const int64_t items = a.n_p * groups;
    for (int64_t it = (int64_t)blockIdx.x * waves + wave; it < items; it += (int64_t)gridDim.x * waves) {
        const int64_t p = it / groups;
        const int v0 = (int)(it - p * groups) * NV_GROUP;
        const int nv = V - v0 < NV_GROUP ? V - v0 : NV_GROUP;
        const int64_t u = a.u_idx[p], i = a.i_idx[p];
        wave_lds_fence();                                      // the reads of the item before are done
        {
            const float *src = a.user.z + u * Su * L;
            for (int e = lane; e < Su * L; e += WAVE) zu[e] = src[e];
            src = a.item.z + i * Si * L;
            for (int e = lane; e < Si * L; e += WAVE) zi[e] = src[e];
            if (lane < L) {
                zu[Su * L + lane] = a.user.z_pad[lane];
                zi[Si * L + lane] = a.item.z_pad[lane];
            }
            if (lane < Su) lgu[lane] = a.user.logit[u * Su + lane];
            if (lane < Si) lgi[lane] = a.item.logit[i * Si + lane];
            if (lane == 0) {
                lgu[Su] = a.user.logit_pad;
                lgi[Si] = a.item.logit_pad;
            }
        }
        float own_u = 0.f, own_i = 0.f;
        const bool has_own_u = a.user.own != nullptr, has_own_i = a.item.own != nullptr;
        if (lane < L) {
            if (has_own_u) own_u = a.user.own[u * L + lane];
            if (has_own_i) own_i = a.item.own[i * L + lane];
        }
        wave_lds_fence();
        const int64_t *du = a.user.drop, *di = a.item.drop;
        uint64_t had_u = 0ull, had_i = 0ull;                   // a side whose mask repeats keeps its pooled vector: the
        float pu_had = 0.f, pi_had = 0.f;                      // same function of the same inputs, so the same bits
        for (int v = 0; v < NV_GROUP; ++v) {
            float x = 0.f;
            if (v < nv) {
                const int64_t at = p * V + v0 + v;
                const uint64_t mu = du ? (uint64_t)du[at] : 0ull, mi = di ? (uint64_t)di[at] : 0ull;
                const uint64_t mask_u = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(mu >> 32)) << 32) |
                                        (uint32_t)__builtin_amdgcn_readfirstlane((int)mu);
                const uint64_t mask_i = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(mi >> 32)) << 32) |
                                        (uint32_t)__builtin_amdgcn_readfirstlane((int)mi);
                if (v == 0 || mask_u != had_u) pu_had = variant_pooled(zu, lgu, sel, mask_u, Su, Ru, L, lane);
                if (v == 0 || mask_i != had_i) pi_had = variant_pooled(zi, lgi, sel, mask_i, Si, Ri, L, lane);
                had_u = mask_u;
                had_i = mask_i;
                float pu = pu_had, pi = pi_had;
                if (has_own_u) pu = pu + own_u;
                if (has_own_i) pi = pi + own_i;
                x = pu * pi;                                   // 0 in the lanes past L
            }
            xs[v * NV_XS + lane] = x;                          // every lane: the tile's columns L .. 63 hold zeros
        }
        wave_lds_fence();
        nv_f32x4 acc[HT];
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) acc[ht] = (nv_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < KT; ++t) {                         // every accumulator sees t ascending
            const float xb = xs[row * NV_XS + 4 * t + kq];
#pragma unroll
            for (int ht = 0; ht < HT; ++ht) acc[ht] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[ht][t], xb, acc[ht], 0, 0, 0);
        }
        float h = 0.f;                                         // h_g of this lane's group g = kq
#pragma unroll
        for (int ht = 0; ht < HT; ++ht)
#pragma unroll
            for (int r = 0; r < 4; ++r) h = __builtin_fmaf(wj[ht][r], __builtin_fmaxf(acc[ht][r] + bj[ht][r], 0.f), h);
        h = h + __shfl_xor(h, 16);                             // h_0 + h_1 | h_2 + h_3
        h = h + __shfl_xor(h, 32);                             // (h_0 + h_1) + (h_2 + h_3)
        if (kq == 0 && row < nv) {
            const float qb = a.q_bias ? a.q_bias[u] : 0.f, cb = a.c_bias ? a.c_bias[i] : 0.f;
            a.out_score[p * V + v0 + row] = (h + qb) + cb;
        }
    }
}

}  // namespace r4r

using namespace r4r;

extern "C" int r4r_narre_logits(const float *z, const int64_t *nb, const float *other_table, int64_t other_rows,
                                const float *W0, const float *b0, const float *w3, const float *b3, float *logit,
                                int64_t N, int S, int L, void *stream) {
    R4R_REQUIRE(N >= 0 && other_rows >= 0, "r4r_narre_logits: negative size (N=%lld other_rows=%lld)", (long long)N,
                (long long)other_rows);
    R4R_REQUIRE(S >= 1 && S <= WI_MAXS, "r4r_narre_logits: S=%d slots outside 1..%d", S, WI_MAXS);
    R4R_REQUIRE(L >= 1 && L <= WI_MAXL, "r4r_narre_logits: L=%d latent units outside 1..%d", L, WI_MAXL);
    if (N == 0) return R4R_OK;
    R4R_REQUIRE(z && nb && W0 && b0 && w3 && b3, "r4r_narre_logits: null pointer among z, nb, W0, b0, w3, b3");
    R4R_REQUIRE(other_table || other_rows == 0, "r4r_narre_logits: null other_table with other_rows=%lld",
                (long long)other_rows);
    R4R_REQUIRE(logit, "r4r_narre_logits: null logit");
    LogitArgs a{z, nb, other_table, other_rows, W0, b0, w3, b3, logit, N, S, L};
    const int64_t want = cdiv(N, LOGIT_WAVES);
    const dim3 grid((unsigned)(want < LOGIT_MAX_BLOCKS ? want : LOGIT_MAX_BLOCKS)), block(LOGIT_WAVES * WAVE);
    hipStream_t st = as_stream(stream);
    if (L <= 16)
        hipLaunchKernelGGL(narre_logits_kernel<16>, grid, block, 0, st, a);
    else if (L <= 32)
        hipLaunchKernelGGL(narre_logits_kernel<32>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(narre_logits_kernel<64>, grid, block, 0, st, a);
    return check_launch("r4r_narre_logits");
}

extern "C" int r4r_narre_whatif(const float *z_u, const float *logit_u, const float *own_u, const float *z_pad_u,
                                float logit_pad_u, int64_t n_u, int S_u, int R_u, const float *z_i, const float *logit_i,
                                const float *own_i, const float *z_pad_i, float logit_pad_i, int64_t n_i, int S_i, int R_i,
                                const int64_t *u_idx, const int64_t *i_idx, const int64_t *drop_u, const int64_t *drop_i,
                                int64_t n_p, int V, const float *q_bias, const float *c_bias, const float *W1,
                                const float *b1, const float *w, int L, float *out_score, void *stream) {
    R4R_REQUIRE(V >= 1, "r4r_narre_whatif: V=%d variants per pair, at least 1", V);
    R4R_REQUIRE(n_p >= 0 && n_p < (1ll << 31) && n_p * V < (1ll << 31), "r4r_narre_whatif: n_p=%lld pairs x V=%d "
                "variants outside 0..2^31-1", (long long)n_p, V);
    if (int rc = variant_require("r4r_narre_whatif", z_u, logit_u, z_pad_u, n_u, S_u, R_u, z_i, logit_i, z_pad_i, n_i, S_i,
                                 R_i, u_idx, i_idx, n_p, W1, b1, w, L))
        return rc;
    if (n_p == 0) return R4R_OK;
    R4R_REQUIRE(out_score, "r4r_narre_whatif: null out_score");
    const size_t slice = variant_slice_floats(S_u, S_i, L);
    const int waves = variant_waves(slice);
    WhatifArgs a{{z_u, logit_u, own_u, z_pad_u, drop_u, logit_pad_u, S_u, R_u},
                 {z_i, logit_i, own_i, z_pad_i, drop_i, logit_pad_i, S_i, R_i},
                 u_idx, i_idx, n_p, V, q_bias, c_bias, W1, b1, w, L, (int)slice, out_score};
    const int64_t want = cdiv(n_p * cdiv(V, NV_GROUP), waves);
    const dim3 grid((unsigned)(want < WI_MAX_BLOCKS ? want : WI_MAX_BLOCKS)), block(waves * WAVE);
    const size_t lds = waves * slice * sizeof(float);
    hipStream_t st = as_stream(stream);
    variant_dispatch(L, [&](auto lt) {
        hipLaunchKernelGGL(narre_whatif_kernel<decltype(lt)::value>, grid, block, lds, st, a);
    });
    return check_launch("r4r_narre_whatif");
}

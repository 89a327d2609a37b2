// NARRE counterfactual search for gfx950 (include/r4r.h, "NARRE counterfactual search"): the fewest reviews whose removal
// moves a pair's eval-mode rating past a target, by a greedy search that runs WHOLE on the device.  A review enters
// NARRE's score only through its own latent and its own attention logit (NARRE.attention, pytorch_models/NARRE.py:53-64;
// the head of NARRE.py:38-46, 115-124), and a removal is the loader's own (`skip`, data.py:144-172, 275-279), so every
// candidate removal at every step is r4r_narre_whatif's variant: a re-selection of slots, a softmax over R logits, a
// pooled vector and the L x L head.  The owner pass (r4r_narre_logits) is paid once; nothing of a tower runs here.
//
// The rule per pair (r4r.h spells it out): the masks start at `start`; column 0 of out_scores is the score under them.
// While the comparison against `target` does not hold and fewer than `budget` removals were made, every slot that is a
// candidate, not yet removed and CURRENTLY SELECTED (among the first R clear slots of its side) is tried as one more
// removed bit; the lowest (direction 0) or highest (direction 1) score is taken, ties to the lowest c (c = slot on the
// user side, 64 + slot on the item side), a NaN never over a number.
//
// Bits: a candidate's score is r4r_narre_whatif's score of the same pair under the same two masks, bit for bit: both
// kernels call csrc/narre_variant_device.h's variant_pooled for the selected list, its softmax and the pooled vector, add
// own, write x = p_u o p_i into a row of the 16 x 66 tile, load W1's fragments in the same layout and end in (h + qb) + cb
// over the same MFMA head.  A column of the MFMA depends on that column's B values only, so a candidate's bits depend on
// its own pair's inputs and its two masks: not on its column, the other candidates, n_p, the grid or the budget.
//
// Shape: one WAVE runs a pair's whole search, grid-strided; the waves of a workgroup are independent, each with its own
// slice of dynamic LDS (narre_whatif_kernel's slice), the pair staged ONCE for all steps.  W1's fragments, b1 and w are
// loaded once per wave, every load before the masks.  Within a step the unchanged side's pooled vector is reused for
// every candidate of the other side; candidates fill the 16 columns of the tile, ceil(candidates / 16) MFMA groups; the
// group's scores are walked in ascending c by wave-uniform reads, the groups in ascending order, so a tie keeps the
// lowest c.  The argument struct is read through kernel_args<>() (common.h); every write is a plain vector store.
#include "common.h"
#include "narre_variant_device.h"

namespace r4r {

constexpr int NS_MAXB = 64;
constexpr int NS_MAX_BLOCKS = 8192;    // beyond, a workgroup's waves loop over pairs

struct SearchSide {                    // one side of a pair
    const float *z, *logit, *own, *z_pad;
    const int64_t *start, *cand;
    float logit_pad;
    int S, R;
};

struct SearchArgs {
    SearchSide user, item;
    const int64_t *u_idx, *i_idx;
    const float *target;
    int64_t n_p;
    int direction, budget;
    const float *q_bias, *c_bias, *W1, *b1, *w;
    int L;
    int slice;                         // floats of one wave's LDS slice
    int32_t *out_order;
    float *out_scores;
    int32_t *out_steps, *out_crossed;
};

__device__ __forceinline__ uint64_t ns_uniform(uint64_t m) {               // a mask every lane holds, as a scalar
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(m >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
}

__device__ __forceinline__ uint64_t ns_slots(int S) { return S >= 64 ? ~0ull : ((1ull << S) - 1ull); }

// The slots of a side the model attends under `mask`: the first R clear slots of 0 .. S - 1, as a wave-uniform mask.
__device__ __forceinline__ uint64_t search_selected(uint64_t mask, int S, int R, int lane) {
    const uint64_t keep = ~mask & ns_slots(S);
    const int rank = __builtin_popcountll(keep & ((1ull << lane) - 1ull));
    return __builtin_amdgcn_ballot_w64(((keep >> lane) & 1ull) && rank < R);
}

// LT: the class of L (L <= 16 LT): 4 LT MFMAs over the input width, LT 16-row tiles of hidden units.
template <int LT>
__global__ __launch_bounds__(NV_MAX_WAVES *WAVE) void narre_search_kernel(const SearchArgs) {
    const SearchArgs &a = kernel_args<SearchArgs>();           // each field an s_load next to its use (common.h)
    constexpr int KT = 4 * LT, HT = LT;
    extern __shared__ __attribute__((aligned(16))) float ns_lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int waves = __builtin_amdgcn_readfirstlane(blockDim.x / WAVE);
    const int L = a.L, B = a.budget;
    const bool up = a.direction != 0;
    const int Su = a.user.S, Si = a.item.S, Ru = a.user.R, Ri = a.item.R;
    // the wave's slice: x tile | sel | user logits | item logits | user rows | item rows
    float *xs = ns_lds + (size_t)wave * a.slice;
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
    const int64_t n_p = a.n_p;
    for (int64_t p = (int64_t)blockIdx.x * waves + wave; p < n_p; p += (int64_t)gridDim.x * waves) {
        const int64_t u = a.u_idx[p], i = a.i_idx[p];
        wave_lds_fence();                                      // the reads of the pair before are done
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
        const float qb = a.q_bias ? a.q_bias[u] : 0.f, cb = a.c_bias ? a.c_bias[i] : 0.f;
        const float target = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a.target[p])));
        // the masks so far, and the slots the search may still remove: wave-uniform, bits >= S and start's bits dropped
        uint64_t mask_u = ns_uniform(a.user.start ? (uint64_t)a.user.start[p] : 0ull) & ns_slots(Su);
        uint64_t mask_i = ns_uniform(a.item.start ? (uint64_t)a.item.start[p] : 0ull) & ns_slots(Si);
        const uint64_t may_u = ns_uniform(a.user.cand ? (uint64_t)a.user.cand[p] : 0ull) & ns_slots(Su) & ~mask_u;
        const uint64_t may_i = ns_uniform(a.item.cand ? (uint64_t)a.item.cand[p] : 0ull) & ns_slots(Si) & ~mask_i;
        wave_lds_fence();
        // the two sides' p' under the masks so far: a side keeps its vector while its mask stands (the same function of
        // the same inputs, so the same bits)
        float pu_now = variant_pooled(zu, lgu, sel, mask_u, Su, Ru, L, lane);
        float pi_now = variant_pooled(zi, lgi, sel, mask_i, Si, Ri, L, lane);
        if (has_own_u) pu_now = pu_now + own_u;
        if (has_own_i) pi_now = pi_now + own_i;
        // column 0 of out_scores: the score under the start masks, as column 0 of a tile
        wave_lds_fence();
        for (int v = 0; v < NV_GROUP; ++v) xs[v * NV_XS + lane] = v == 0 ? pu_now * pi_now : 0.f;
        wave_lds_fence();
        float score = (variant_head<LT>(xs, wf, bj, wj, row, kq) + qb) + cb;
        score = lane_value(score, 0);
        float *scores = a.out_scores + p * (B + 1);
        int32_t *order = a.out_order + p * B;
        if (lane == 0) scores[0] = score;
        int steps = 0;
        bool crossed = up ? score > target : score < target;
        while (!crossed && steps < B) {
            uint64_t left_u = search_selected(mask_u, Su, Ru, lane) & may_u & ~mask_u;
            uint64_t left_i = search_selected(mask_i, Si, Ri, lane) & may_i & ~mask_i;
            if (!(left_u | left_i)) break;                     // no candidate is left
            bool have = false;
            float best = 0.f;
            int best_c = -1;
            while (left_u | left_i) {                          // one MFMA group: the next 16 candidates, c ascending
                int nv = 0, my_c = -1;
                wave_lds_fence();                              // the tile reads of the group before are done
                for (int v = 0; v < NV_GROUP; ++v) {
                    float x = 0.f;
                    if (left_u | left_i) {
                        int c;
                        if (left_u) {
                            const int s = __builtin_ctzll(left_u);
                            left_u &= left_u - 1ull;
                            c = s;
                            float pu = variant_pooled(zu, lgu, sel, mask_u | (1ull << s), Su, Ru, L, lane);
                            if (has_own_u) pu = pu + own_u;
                            x = pu * pi_now;                   // 0 in the lanes past L
                        } else {
                            const int s = __builtin_ctzll(left_i);
                            left_i &= left_i - 1ull;
                            c = 64 + s;
                            float pi = variant_pooled(zi, lgi, sel, mask_i | (1ull << s), Si, Ri, L, lane);
                            if (has_own_i) pi = pi + own_i;
                            x = pu_now * pi;
                        }
                        if (lane == v) my_c = c;
                        nv = v + 1;
                    }
                    xs[v * NV_XS + lane] = x;                  // every lane: the tile's columns L .. 63 hold zeros
                }
                wave_lds_fence();
                const float got = (variant_head<LT>(xs, wf, bj, wj, row, kq) + qb) + cb;     // lanes 0 .. 15: column = lane
                for (int v = 0; v < nv; ++v) {                 // ascending c: a later candidate must be strictly better
                    const float s = lane_value(got, v);
                    const bool better = !have || (best != best && s == s) || (up ? s > best : s < best);
                    if (better) {
                        have = true;
                        best = s;
                        best_c = __builtin_amdgcn_readlane(my_c, v);
                    }
                }
            }
            // the best candidate is taken, whichever way it moves the score
            if (best_c < 64) {
                mask_u |= 1ull << best_c;
                pu_now = variant_pooled(zu, lgu, sel, mask_u, Su, Ru, L, lane);
                if (has_own_u) pu_now = pu_now + own_u;
            } else {
                mask_i |= 1ull << (best_c - 64);
                pi_now = variant_pooled(zi, lgi, sel, mask_i, Si, Ri, L, lane);
                if (has_own_i) pi_now = pi_now + own_i;
            }
            score = best;
            if (lane == 0) {
                order[steps] = best_c;
                scores[steps + 1] = score;
            }
            ++steps;
            crossed = up ? score > target : score < target;
        }
        for (int j = steps + lane; j < B; j += WAVE) {         // beyond the last step: no candidate, the last score
            order[j] = -1;
            scores[j + 1] = score;
        }
        if (lane == 0) {
            a.out_steps[p] = steps;
            a.out_crossed[p] = crossed ? 1 : 0;
        }
    }
}

}  // namespace r4r

using namespace r4r;

extern "C" int r4r_narre_search(const float *z_u, const float *logit_u, const float *own_u, const float *z_pad_u,
                                float logit_pad_u, int64_t n_u, int S_u, int R_u, const float *z_i, const float *logit_i,
                                const float *own_i, const float *z_pad_i, float logit_pad_i, int64_t n_i, int S_i, int R_i,
                                const int64_t *u_idx, const int64_t *i_idx, const int64_t *start_u, const int64_t *start_i,
                                const int64_t *cand_u, const int64_t *cand_i, const float *target, int direction,
                                int budget, int64_t n_p, const float *q_bias, const float *c_bias, const float *W1,
                                const float *b1, const float *w, int L, int32_t *out_order, float *out_scores,
                                int32_t *out_steps, int32_t *out_crossed, void *stream) {
    R4R_REQUIRE(budget >= 1 && budget <= NS_MAXB, "r4r_narre_search: budget=%d removals outside 1..%d", budget, NS_MAXB);
    R4R_REQUIRE(direction == 0 || direction == 1, "r4r_narre_search: direction=%d is neither 0 (down) nor 1 (up)",
                direction);
    R4R_REQUIRE(n_p >= 0 && n_p < (1ll << 31) && n_p * (budget + 1) < (1ll << 31), "r4r_narre_search: n_p=%lld pairs x "
                "(budget=%d + 1) scores outside 0..2^31-1", (long long)n_p, budget);
    if (int rc = variant_require("r4r_narre_search", z_u, logit_u, z_pad_u, n_u, S_u, R_u, z_i, logit_i, z_pad_i, n_i, S_i,
                                 R_i, u_idx, i_idx, n_p, W1, b1, w, L))
        return rc;
    if (n_p == 0) return R4R_OK;
    R4R_REQUIRE(target, "r4r_narre_search: null target");
    R4R_REQUIRE(out_order && out_scores && out_steps && out_crossed,
                "r4r_narre_search: null pointer among out_order, out_scores, out_steps, out_crossed");
    const size_t slice = variant_slice_floats(S_u, S_i, L);
    const int waves = variant_waves(slice);
    SearchArgs a{{z_u, logit_u, own_u, z_pad_u, start_u, cand_u, logit_pad_u, S_u, R_u},
                 {z_i, logit_i, own_i, z_pad_i, start_i, cand_i, logit_pad_i, S_i, R_i},
                 u_idx, i_idx, target, n_p, direction, budget, q_bias, c_bias, W1, b1, w, L, (int)slice,
                 out_order, out_scores, out_steps, out_crossed};
    const int64_t want = cdiv(n_p, waves);
    const dim3 grid((unsigned)(want < NS_MAX_BLOCKS ? want : NS_MAX_BLOCKS)), block(waves * WAVE);
    const size_t lds = waves * slice * sizeof(float);
    hipStream_t st = as_stream(stream);
    variant_dispatch(L, [&](auto lt) {
        hipLaunchKernelGGL(narre_search_kernel<decltype(lt)::value>, grid, block, lds, st, a);
    });
    return check_launch("r4r_narre_search");
}

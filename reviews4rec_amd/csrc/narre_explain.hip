// NARRE explanations for gfx950: the eval-mode review attention for R <= 64 reviews and L <= 64 latent units that KEEPS
// its weights -- the pooled vector, the softmax weights of every slot and the K heaviest live slots of every owner, one
// launch, forward only (include/r4r.h, "NARRE explanations").
//
// Reference behaviour restated: NARRE.attention, pytorch_models/NARRE.py:53-64, in eval mode, with the scorer of
// NARRE.py:24-36 exactly as csrc/narre.hip restates it: h = relu(W0 [z_r ; other_r] + b0), a = softmax_R(w3 . h + b3),
// out = sum_r a_r z_r.  Padded (all-zero) reviews are NOT masked out of the softmax, like the reference; they are only
// kept off the lists.
//
// One WAVE per owner; a workgroup is EX_WAVES independent waves that share one LDS image of W0 (staged once, then each
// wave walks its own owners: the only workgroup barrier is the one after the staging).  Steps 1 to 3 are the functions of
// csrc/narre_attn_device.h; the what-if logits (narre_whatif.hip) call step 1 too, and the attention Jacobian
// (narre_pair.hip) keeps the same sequence inline: their logits, attn and out have this kernel's bits.  Per owner:
//   1. EX_SLOTS = 5 slots at a time, the logits (attn_group_logits): 20 FMAs per 6 LDS reads, a slot's logit independent
//      of where in a group it sits.
//   2. lane r holds slot r's logit: the softmax (attn_softmax) -> a_r.
//   3. lane l sums a_r z_r over the slots in ascending order (attn_pooled), plus the owner's own row.
//   4. lane r counts the LIVE slots ahead of it (weight descending, ties by ascending slot) and, below K, stores itself
//      at that place: R <= 64 is one wave's worth of slots, so there is no sort and no insertion chain.
// Everything an owner's outputs depend on is that owner's inputs and the weights: not N, not the grid, not K, not which
// outputs are asked for.  The problem is R L 2L MACs per owner (82k at 10 x 64): launch and latency bound, no MFMA.
// The argument struct is taken by value, as before the owner pass moved into the header: this kernel spills no scalar.
#include "common.h"
#include "narre_attn_device.h"

namespace r4r {

constexpr int EX_MAXR = 64, EX_MAXL = 64;
#ifndef R4R_EX_WAVES
#define R4R_EX_WAVES 12                // (measured: DESIGN.md 4.22 has 4, 8, 12 and 16)
#endif
constexpr int EX_WAVES = R4R_EX_WAVES; // waves (= owners in flight) per workgroup, sharing one image of W0
#ifndef R4R_EX_SLOTS
#define R4R_EX_SLOTS 5                 // (an A/B build may set another: `make variant EXTRA=-DR4R_EX_SLOTS=4`)
#endif
constexpr int EX_SLOTS = R4R_EX_SLOTS; // slots per staged group: R = 10, the catalogue's only R, is two groups of five
constexpr int EX_MAX_BLOCKS = 1024;    // beyond, a workgroup's waves loop over owners

struct ExplainArgs {
    const float *z;
    const int64_t *nb;
    const float *other_table;
    int64_t other_rows;
    const float *own_table;
    const int64_t *owner;
    const int32_t *live;
    const float *W0, *b0, *w3, *b3;
    float *out, *attn;
    int32_t *top_slot;
    float *top_w;
    int K;
    int64_t N;
    int R, L;
};

// LMAX: the class of L (L <= LMAX) -- it fixes the LDS strides, nothing of the arithmetic.
template <int LMAX>
__global__ __launch_bounds__(EX_WAVES *WAVE) void narre_explain_kernel(const ExplainArgs a) {
    __shared__ __attribute__((aligned(16))) float w0s[LMAX * ATTN_WS<LMAX>];
    __shared__ __attribute__((aligned(16))) float cats[EX_WAVES][EX_SLOTS * ATTN_CS<LMAX>];
    const int R = a.R, L = a.L;
    attn_stage_w0<LMAX>(w0s, a.W0, L, EX_WAVES * WAVE);
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    float *cat = cats[wave];
    const AttnLane ln = attn_lane<LMAX>(w0s, a.b0, a.w3, a.b3, L, lane);
    for (int64_t n = (int64_t)blockIdx.x * EX_WAVES + wave; n < a.N; n += (int64_t)gridDim.x * EX_WAVES) {
        const float *zn = a.z + n * R * L;
        const int64_t *nbn = a.nb + n * R;
        float sc = -INFINITY;                                  // lane r: the logit of slot r
        for (int r0 = 0; r0 < R; r0 += EX_SLOTS)
            attn_group_logits<LMAX, EX_SLOTS>(cat, zn, nbn, a.other_table, a.other_rows, r0, R, L, ln, lane, sc);
        const float w = attn_softmax(sc, R, lane);         // lane r: a_r; 0 in the lanes past R
        if (a.attn && lane < R) a.attn[n * R + lane] = w;
        if (a.out) {
            float o = attn_pooled(w, zn, R, L, lane);
            if (lane < L) {
                if (a.own_table) o += a.own_table[a.owner[n] * L + lane];
                a.out[n * L + lane] = o;
            }
        }
        if (a.K > 0) {
            int lv = R;
            if (a.live) {
                lv = __builtin_amdgcn_readfirstlane(a.live[n]);
                lv = lv < 0 ? 0 : (lv > R ? R : lv);
            }
            int place = 0;
            for (int r = 0; r < lv; ++r) {
                const float o = lane_value(w, r);
                place += (o > w || (o == w && r < lane)) ? 1 : 0;
            }
            if (lane < lv && place < a.K) {
                a.top_slot[n * a.K + place] = lane;
                a.top_w[n * a.K + place] = w;
            }
            if (lane >= lv && lane < a.K) {                    // the places beyond min(K, live)
                a.top_slot[n * a.K + lane] = -1;
                a.top_w[n * a.K + lane] = 0.f;
            }
        }
    }
}

}  // namespace r4r

using namespace r4r;

extern "C" int r4r_narre_explain(const float *z, const int64_t *nb, const float *other_table, int64_t other_rows,
                                 const float *own_table, const int64_t *owner, const int32_t *live,
                                 const float *W0, const float *b0, const float *w3, const float *b3,
                                 float *out, float *attn, int32_t *top_slot, float *top_w, int K,
                                 int64_t N, int R, int L, void *stream) {
    R4R_REQUIRE(N >= 0 && other_rows >= 0, "narre_explain: negative size (N=%lld other_rows=%lld)", (long long)N,
                (long long)other_rows);
    R4R_REQUIRE(R > 0 && R <= EX_MAXR && L > 0 && L <= EX_MAXL, "narre_explain: R=%d L=%d outside 1..64", R, L);
    R4R_REQUIRE(K >= 0 && K <= R, "narre_explain: K=%d outside 0..R=%d", K, R);
    R4R_REQUIRE((own_table == nullptr) == (owner == nullptr), "narre_explain: own_table and owner go together");
    R4R_REQUIRE((top_slot == nullptr) == (top_w == nullptr), "narre_explain: top_slot and top_w go together");
    if (N == 0) return R4R_OK;
    R4R_REQUIRE(z && nb && W0 && b0 && w3 && b3, "narre_explain: null pointer");
    R4R_REQUIRE(other_table || other_rows == 0, "narre_explain: null other_table with other_rows=%lld",
                (long long)other_rows);
    R4R_REQUIRE(K == 0 || top_slot, "narre_explain: K=%d without top_slot / top_w", K);
    R4R_REQUIRE(out || attn || K > 0, "narre_explain: no output asked for (out, attn and the lists are all null)");
    ExplainArgs a{z, nb, other_table, other_rows, own_table, owner, live, W0, b0, w3, b3, out, attn,
                  top_slot, top_w, K, N, R, L};
    const int64_t want = cdiv(N, EX_WAVES);
    const unsigned blocks = (unsigned)(want < EX_MAX_BLOCKS ? want : EX_MAX_BLOCKS);
    hipStream_t st = as_stream(stream);
    if (L <= 16)
        narre_explain_kernel<16><<<blocks, EX_WAVES * WAVE, 0, st>>>(a);
    else if (L <= 32)
        narre_explain_kernel<32><<<blocks, EX_WAVES * WAVE, 0, st>>>(a);
    else
        narre_explain_kernel<64><<<blocks, EX_WAVES * WAVE, 0, st>>>(a);
    return check_launch("narre_explain");
}

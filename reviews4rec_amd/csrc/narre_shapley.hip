// NARRE Shapley values for gfx950 (include/r4r.h, "NARRE Shapley values"): how much of a pair's eval-mode rating each
// attended review carries, as the exact Shapley value of the game "which of the players' reviews are present".  A review
// enters NARRE's score only through its own latent and its own attention logit (NARRE.attention,
// pytorch_models/NARRE.py:53-64; the head of NARRE.py:38-46, 115-124), and an absent review is the loader's own removal
// (`skip`, data.py:144-172, 275-279), so a coalition is one variant of r4r_narre_whatif: a re-selection of slots, a
// softmax over R logits, a pooled vector and the L x L head.  The owner pass (r4r_narre_logits) is paid once; nothing of
// a tower runs here.  No mask and no score of a coalition goes through memory (out_values apart, when asked for): a
// coalition's masks are formed from its number in registers, its score is folded into n running sums.
//
// The rule per pair (r4r.h spells it out): the players are the set bits of play, less start's and those >= S, the user
// side's ascending first, then the item side's, the lowest-numbered P of them; coalition c has bit t set when player t is
// PRESENT, its masks are start | (the players whose bit is clear).  phi_t = sum over c of coef_t(c) (v(c) - v(2^n - 1)).
//
// Bits of a value: v(c) is r4r_narre_whatif's score of the same pair under the same two masks, bit for bit: this kernel
// calls csrc/narre_variant_device.h's variant_pooled and variant_head as narre_search.hip does -- own added to the
// pooled vector, x = p_u o p_i into a row of the 16 x 66 tile, W1's fragments in the same layout, (h + qb) + cb.  A
// column of the MFMA depends on that column's B values only.
//
// Shape: one WAVE per (pair, chunk of SH_CHUNK = 1,024 consecutive coalitions), grid-strided; the waves of a workgroup are
// independent, each with its own slice of dynamic LDS (narre_whatif_kernel's slice), the pair staged ONCE per wave, W1's
// fragments loaded once per wave.  A wave first scores the pair under start alone (v(2^n - 1), the centre), then walks
// its chunk 16 coalitions a tile: lane s forms bit s of either mask from c and its own player number (one ballot a
// side); a side whose mask repeats keeps its pooled vector, so in a one-side game the other side is pooled once per
// wave and in a two-side game the item side once per 2^n_u coalitions.  Lane j of 0 .. 15 then folds column j's value
// into its 16 float64 sums; at the end of the chunk the 16 lanes' sums meet in an xor butterfly.  With P <= 10 a pair is
// one chunk and the wave writes phi; beyond, the chunk sums go to the caller's scratch and narre_shapley_combine adds them
// in ascending chunk order: no atomics, and a pair's bits do not depend on who else is in the call.
// The argument struct is read through kernel_args<>() (common.h); every write is a plain vector store.
#include "common.h"
#include "narre_variant_device.h"

namespace r4r {

constexpr int SH_MAXP = 16;            // players of one pair
constexpr int SH_CHUNK_LOG = 10;       // a wave's chunk: 2^10 coalitions, 64 tiles
constexpr int SH_MAX_BLOCKS = 8192;    // beyond, a workgroup's waves loop over (pair, chunk)
constexpr int SH_COMBINE_THREADS = 256;

struct ShapleySide {                   // one side of a pair
    const float *z, *logit, *own, *z_pad;
    const int64_t *start, *play;
    float logit_pad;
    int S, R;
    float *out_phi;
};

struct ShapleyArgs {
    ShapleySide user, item;
    const int64_t *u_idx, *i_idx;
    int64_t n_p;
    int P;
    int chunks;                        // chunks of a pair with P players: max(1, 2^(P - 10))
    const float *q_bias, *c_bias, *W1, *b1, *w;
    int L;
    int slice;                         // floats of one wave's LDS slice
    float *out_base, *out_empty;
    int32_t *out_n;
    float *out_values;
    double *scratch;
};

// The Shapley weights, formed in float64 and rounded to fp32 once: a[n][k] = (k - 1)! (n - k)! / n! = 1 / (n C(n-1, k-1))
// for 1 <= k <= n, 0 elsewhere.  coef_t(c) with k = |c| is a[n][k] for t in c and -a[n][k + 1] for t not in c.
struct ShapleyWeights {
    float a[SH_MAXP + 1][SH_MAXP + 2];
};

constexpr ShapleyWeights shapley_weights() {
    ShapleyWeights w{};
    for (int n = 1; n <= SH_MAXP; ++n) {
        double C = 1.0;                                        // C(n - 1, k - 1): small integers, every step exact
        for (int k = 1; k <= n; ++k) {
            w.a[n][k] = (float)(1.0 / ((double)n * C));
            C = C * (double)(n - k) / (double)k;
        }
    }
    return w;
}

__device__ const ShapleyWeights SH_W = shapley_weights();

__host__ __device__ __forceinline__ uint64_t sh_slots(int S) { return S >= 64 ? ~0ull : ((1ull << S) - 1ull); }

// The lowest k set bits of m.
__host__ __device__ __forceinline__ uint64_t sh_lowest(uint64_t m, int k) {
    while (__builtin_popcountll(m) > k) m &= ~(1ull << (63 - __builtin_clzll(m)));
    return m;
}

// The players of a pair: start's bits and the bits >= S dropped, the user side's first, the lowest-numbered P in all.
__host__ __device__ __forceinline__ void shapley_players(uint64_t start_u, uint64_t start_i, uint64_t play_u,
                                                         uint64_t play_i, int Su, int Si, int P, uint64_t &pl_u,
                                                         uint64_t &pl_i) {
    pl_u = sh_lowest(play_u & sh_slots(Su) & ~start_u, P);
    pl_i = sh_lowest(play_i & sh_slots(Si) & ~start_i, P - __builtin_popcountll(pl_u));
}

__device__ __forceinline__ uint64_t sh_uniform(uint64_t m) {               // a mask every lane holds, as a scalar
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(m >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
}

__device__ __forceinline__ double sh_first(double v) {                     // lane 0's value, as a scalar
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    return __builtin_bit_cast(double, sh_uniform(b));
}

// LT: the class of L (L <= 16 LT): 4 LT MFMAs over the input width, LT 16-row tiles of hidden units.
template <int LT>
__global__ __launch_bounds__(NV_MAX_WAVES *WAVE) void narre_shapley_kernel(const ShapleyArgs) {
    const ShapleyArgs &a = kernel_args<ShapleyArgs>();         // each field an s_load next to its use (common.h)
    constexpr int KT = 4 * LT, HT = LT;
    extern __shared__ __attribute__((aligned(16))) float sh_lds[];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int waves = __builtin_amdgcn_readfirstlane(blockDim.x / WAVE);
    const int L = a.L, P = a.P, chunks = a.chunks;
    const int Su = a.user.S, Si = a.item.S, Ru = a.user.R, Ri = a.item.R;
    // the wave's slice: x tile | sel | user logits | item logits | user rows | item rows
    float *xs = sh_lds + (size_t)wave * a.slice;
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
    const uint64_t below = (1ull << lane) - 1ull;
    const int64_t items = a.n_p * chunks;
    for (int64_t it = (int64_t)blockIdx.x * waves + wave; it < items; it += (int64_t)gridDim.x * waves) {
        const int64_t p = it / chunks;
        const int q = (int)(it - p * chunks);
        // the masks of every coalition, and the players: wave-uniform, bits >= S and start's bits dropped
        const uint64_t st_u = sh_uniform(a.user.start ? (uint64_t)a.user.start[p] : 0ull) & sh_slots(Su);
        const uint64_t st_i = sh_uniform(a.item.start ? (uint64_t)a.item.start[p] : 0ull) & sh_slots(Si);
        uint64_t pl_u, pl_i;
        shapley_players(st_u, st_i, sh_uniform(a.user.play ? (uint64_t)a.user.play[p] : 0ull),
                        sh_uniform(a.item.play ? (uint64_t)a.item.play[p] : 0ull), Su, Si, P, pl_u, pl_i);
        const int nu = __builtin_popcountll(pl_u), n = nu + __builtin_popcountll(pl_i);
        const int ncoal = 1 << n, c_lo = q << SH_CHUNK_LOG;
        if (c_lo >= ncoal) continue;                           // a pair of fewer players has fewer chunks
        const int c_hi = c_lo + (1 << SH_CHUNK_LOG) < ncoal ? c_lo + (1 << SH_CHUNK_LOG) : ncoal;
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
        const float qb = a.q_bias ? a.q_bias[u] : 0.f, cb = a.c_bias ? a.c_bias[i] : 0.f;
        // lane s: is slot s a player of its side, and which (0 .. 15)
        const bool is_u = (pl_u >> lane) & 1ull, is_i = (pl_i >> lane) & 1ull;
        const int tu = __builtin_popcountll(pl_u & below) & 15, ti = (nu + __builtin_popcountll(pl_i & below)) & 15;
        // lane k: a[n][k]
        const float wk = lane <= SH_MAXP + 1 ? SH_W.a[n][lane] : 0.f;
        wave_lds_fence();
        // the centre v(2^n - 1): every player present, the masks are start's; a side keeps its vector while its mask
        // repeats (the same function of the same inputs, so the same bits)
        uint64_t had_u = st_u, had_i = st_i;
        float pu_had = variant_pooled(zu, lgu, sel, st_u, Su, Ru, L, lane);
        float pi_had = variant_pooled(zi, lgi, sel, st_i, Si, Ri, L, lane);
        if (has_own_u) pu_had = pu_had + own_u;
        if (has_own_i) pi_had = pi_had + own_i;
        wave_lds_fence();
        for (int v = 0; v < NV_GROUP; ++v) xs[v * NV_XS + lane] = v == 0 ? pu_had * pi_had : 0.f;
        wave_lds_fence();
        const float vbase = lane_value((variant_head<LT>(xs, wf, bj, wj, row, kq) + qb) + cb, 0);
        float vempty = vbase;                                  // v(0); with no player the one coalition is the centre
        float *values = a.out_values ? a.out_values + (p << P) : nullptr;
        double acc[SH_MAXP];
#pragma unroll
        for (int t = 0; t < SH_MAXP; ++t) acc[t] = 0.0;
        if (n == 0) {
            if (values && lane == 0) values[0] = vbase;
        } else {
            for (int c0 = c_lo; c0 < c_hi; c0 += NV_GROUP) {   // one MFMA group: 16 coalitions, c ascending
                wave_lds_fence();                              // the tile reads of the group before are done
                for (int v = 0; v < NV_GROUP; ++v) {
                    float x = 0.f;
                    const uint32_t c = (uint32_t)(c0 + v);
                    if (c0 + v < c_hi) {
                        const uint64_t mask_u = st_u | __builtin_amdgcn_ballot_w64(is_u && !((c >> tu) & 1u));
                        const uint64_t mask_i = st_i | __builtin_amdgcn_ballot_w64(is_i && !((c >> ti) & 1u));
                        if (mask_u != had_u) {
                            pu_had = variant_pooled(zu, lgu, sel, mask_u, Su, Ru, L, lane);
                            if (has_own_u) pu_had = pu_had + own_u;
                            had_u = mask_u;
                        }
                        if (mask_i != had_i) {
                            pi_had = variant_pooled(zi, lgi, sel, mask_i, Si, Ri, L, lane);
                            if (has_own_i) pi_had = pi_had + own_i;
                            had_i = mask_i;
                        }
                        x = pu_had * pi_had;                   // 0 in the lanes past L
                    }
                    xs[v * NV_XS + lane] = x;                  // every lane: the tile's columns L .. 63 hold zeros
                }
                wave_lds_fence();
                const float got = (variant_head<LT>(xs, wf, bj, wj, row, kq) + qb) + cb;     // lanes 0 .. 15: column = lane
                const int cl = c0 + lane;
                const bool mine = lane < NV_GROUP && cl < c_hi;
                if (values && mine) values[cl] = got;
                if (c0 == 0) vempty = lane_value(got, 0);
                // lane j: column j's centred value into the n sums, in float64
                const int k = __builtin_popcount((uint32_t)cl);
                const float w_in = __shfl(wk, k), w_out = -__shfl(wk, k + 1);
                const double d = mine ? (double)got - (double)vbase : 0.0;
#pragma unroll
                for (int t = 0; t < SH_MAXP; ++t)
                    acc[t] = __builtin_fma((double)(((cl >> t) & 1) ? w_in : w_out), d, acc[t]);
            }
#pragma unroll
            for (int t = 0; t < SH_MAXP; ++t) {
                if (t < n) {                                   // the 16 lanes' sums: xor 1, 2, 4, 8
                    double s = acc[t];
                    s = s + __shfl_xor(s, 1);
                    s = s + __shfl_xor(s, 2);
                    s = s + __shfl_xor(s, 4);
                    s = s + __shfl_xor(s, 8);
                    acc[t] = sh_first(s);
                }
            }
        }
        if (q == 0 && lane == 0) {
            a.out_base[p] = vbase;
            a.out_empty[p] = vempty;
            a.out_n[p] = n;
        }
        if (chunks == 1) {                                     // the pair's one chunk: phi by slot, +0.0f at a slot that is no player
            double mu = 0.0, mi = 0.0;
#pragma unroll
            for (int t = 0; t < SH_MAXP; ++t) {
                mu = (is_u && tu == t) ? acc[t] : mu;
                mi = (is_i && ti == t) ? acc[t] : mi;
            }
            if (a.user.out_phi && lane < Su) a.user.out_phi[p * Su + lane] = (float)(0.0 + mu);
            if (a.item.out_phi && lane < Si) a.item.out_phi[p * Si + lane] = (float)(0.0 + mi);
        } else {
            double *part = a.scratch + (p * chunks + q) * P;
#pragma unroll
            for (int t = 0; t < SH_MAXP; ++t)
                if (t < n && lane == 0) part[t] = acc[t];
        }
    }
}

// The chunk sums of a pair added in ascending chunk order, from 0.0, and rounded once: one thread per (pair, slot of
// either side).
__global__ __launch_bounds__(SH_COMBINE_THREADS) void narre_shapley_combine(const ShapleyArgs) {
    const ShapleyArgs &a = kernel_args<ShapleyArgs>();
    const int Su = a.user.S, Si = a.item.S, P = a.P, chunks = a.chunks;
    const int64_t at = (int64_t)blockIdx.x * SH_COMBINE_THREADS + threadIdx.x;
    const int64_t p = at / (Su + Si);
    if (p >= a.n_p) return;
    const int j = (int)(at - p * (Su + Si));
    const uint64_t st_u = (a.user.start ? (uint64_t)a.user.start[p] : 0ull) & sh_slots(Su);
    const uint64_t st_i = (a.item.start ? (uint64_t)a.item.start[p] : 0ull) & sh_slots(Si);
    uint64_t pl_u, pl_i;
    shapley_players(st_u, st_i, a.user.play ? (uint64_t)a.user.play[p] : 0ull, a.item.play ? (uint64_t)a.item.play[p] : 0ull,
                    Su, Si, P, pl_u, pl_i);
    const int nu = __builtin_popcountll(pl_u), n = nu + __builtin_popcountll(pl_i);
    const bool user = j < Su;
    const int s = user ? j : j - Su;
    float *out = user ? a.user.out_phi : a.item.out_phi;
    if (!out) return;
    const uint64_t pl = user ? pl_u : pl_i;
    double sum = 0.0;
    if ((pl >> s) & 1ull) {
        const int t = (user ? 0 : nu) + __builtin_popcountll(pl & ((1ull << s) - 1ull));
        const int mine = n > SH_CHUNK_LOG ? 1 << (n - SH_CHUNK_LOG) : 1;
        const double *part = a.scratch + p * chunks * P + t;
        for (int q = 0; q < mine; ++q) sum = sum + part[(int64_t)q * P];
    }
    out[p * (user ? Su : Si) + s] = (float)sum;
}

}  // namespace r4r

using namespace r4r;

extern "C" int r4r_narre_shapley(const float *z_u, const float *logit_u, const float *own_u, const float *z_pad_u,
                                 float logit_pad_u, int64_t n_u, int S_u, int R_u, const float *z_i, const float *logit_i,
                                 const float *own_i, const float *z_pad_i, float logit_pad_i, int64_t n_i, int S_i,
                                 int R_i, const int64_t *u_idx, const int64_t *i_idx, const int64_t *start_u,
                                 const int64_t *start_i, const int64_t *play_u, const int64_t *play_i, int P, int64_t n_p,
                                 const float *q_bias, const float *c_bias, const float *W1, const float *b1, const float *w,
                                 int L, float *out_phi_u, float *out_phi_i, float *out_base, float *out_empty,
                                 int32_t *out_n, float *out_values, double *scratch, void *stream) {
    R4R_REQUIRE(P >= 1 && P <= SH_MAXP, "r4r_narre_shapley: P=%d players outside 1..%d", P, SH_MAXP);
    R4R_REQUIRE(n_p >= 0 && n_p < (1ll << 31), "r4r_narre_shapley: n_p=%lld pairs outside 0..2^31-1", (long long)n_p);
    R4R_REQUIRE(!out_values || (n_p << P) < (1ll << 31), "r4r_narre_shapley: n_p=%lld pairs x 2^P=%d out_values outside "
                "0..2^31-1", (long long)n_p, 1 << P);
    if (int rc = variant_require("r4r_narre_shapley", z_u, logit_u, z_pad_u, n_u, S_u, R_u, z_i, logit_i, z_pad_i, n_i,
                                 S_i, R_i, u_idx, i_idx, n_p, W1, b1, w, L))
        return rc;
    if (n_p == 0) return R4R_OK;
    R4R_REQUIRE(out_base && out_empty && out_n, "r4r_narre_shapley: null pointer among out_base, out_empty, out_n");
    R4R_REQUIRE(out_phi_u || !play_u, "r4r_narre_shapley: null out_phi_u with players on the user side");
    R4R_REQUIRE(out_phi_i || !play_i, "r4r_narre_shapley: null out_phi_i with players on the item side");
    const int chunks = P > SH_CHUNK_LOG ? 1 << (P - SH_CHUNK_LOG) : 1;
    R4R_REQUIRE(scratch || chunks == 1, "r4r_narre_shapley: null scratch with P=%d > %d (n_p x 2^(P-%d) x P doubles)", P,
                SH_CHUNK_LOG, SH_CHUNK_LOG);
    const size_t slice = variant_slice_floats(S_u, S_i, L);
    const int waves = variant_waves(slice);
    ShapleyArgs a{{z_u, logit_u, own_u, z_pad_u, start_u, play_u, logit_pad_u, S_u, R_u, out_phi_u},
                  {z_i, logit_i, own_i, z_pad_i, start_i, play_i, logit_pad_i, S_i, R_i, out_phi_i},
                  u_idx, i_idx, n_p, P, chunks, q_bias, c_bias, W1, b1, w, L, (int)slice,
                  out_base, out_empty, out_n, out_values, scratch};
    const int64_t want = cdiv(n_p * chunks, waves);
    const dim3 grid((unsigned)(want < SH_MAX_BLOCKS ? want : SH_MAX_BLOCKS)), block(waves * WAVE);
    const size_t lds = waves * slice * sizeof(float);
    hipStream_t st = as_stream(stream);
    variant_dispatch(L, [&](auto lt) {
        hipLaunchKernelGGL(narre_shapley_kernel<decltype(lt)::value>, grid, block, lds, st, a);
    });
    if (int rc = check_launch("r4r_narre_shapley")) return rc;
    if (chunks > 1) {
        const dim3 cgrid((unsigned)cdiv(n_p * (S_u + S_i), SH_COMBINE_THREADS));
        hipLaunchKernelGGL(narre_shapley_combine, cgrid, dim3(SH_COMBINE_THREADS), 0, st, a);
        return check_launch("r4r_narre_shapley");
    }
    return R4R_OK;
}

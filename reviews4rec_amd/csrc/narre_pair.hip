// NARRE pair gradients for gfx950 (include/r4r.h, "NARRE pair gradients"): the gradient of ONE user-item score through
// the softmax of NARRE's review attention, split into a per-owner pass (r4r_narre_attn_jac) and a per-pair pass
// (r4r_narre_pair_grad), so that no pair repeats a review's matrix work.
//
// Reference behaviour restated: NARRE.attention, pytorch_models/NARRE.py:53-64, in eval mode, the scorer of
// NARRE.py:24-36 and the head of NARRE.py:38-46, 115-124 (dropout is the identity in eval mode).  Per side, with
// z_r = fc pooled_r + fc.bias:  pre_r = W0 [z_r ; e_r] + b0,  a = softmax_R(w3 . relu(pre_r) + b3),  o = sum_r a_r z_r,
// p = o + own row;  x = p_u o p_i,  t = W1 x + b1,  score = w . relu(t) + scalars.
//
// Owner pass: narre_explain.hip's kernel shape -- one WAVE per owner, JAC_WAVES waves share one LDS image of W0 -- and
// the instruction sequence of csrc/narre_attn_device.h for the logits, the softmax and the pooled vector, so that attn and
// out have r4r_narre_explain's bits.  It stands inline here, with the ReLU ballot in its epilogue: as calls of the shared
// functions this kernel measured 3 % slower at L = 64.  The ReLU masks of a slot (one bit per hidden unit) are a ballot kept in lane r's registers.
// Then per slot r: lane j chains D_r[j] = sum_m [pre_rm > 0] w3_m W0[m, j] over m ascending out of the LDS image (row m,
// consecutive j: conflict free), dz_r is the fixed-order wave sum of D_r[j] z_r[j], and E_r = D_r fc is cols_matvec with
// D_r as an LDS broadcast (the wave's staging rows are free by then).
// Pair pass: pair_grad.hip's kernel shape -- one WAVE per pair, PAIR_WAVES independent waves, grid-strided, a pair's
// vectors in the wave's own LDS slice, the matrices read from global memory (L2 / the vector cache serve them).
// Both kernels read their argument struct through kernel_args<>() (common.h).
#include "common.h"

namespace r4r {

constexpr int NP_MAXR = 64, NP_MAXL = 64, NP_MAXF = 112;
constexpr int JAC_WAVES = 8;           // waves (= owners in flight) per workgroup, sharing one image of W0
constexpr int JAC_SLOTS = 5;           // slots per staged group: narre_explain.hip's EX_SLOTS (the logits' bits do not
                                       // depend on it, the speed at R = 10 does)
constexpr int JAC_MAX_BLOCKS = 1024;   // beyond, a workgroup's waves loop over owners
constexpr int PAIR_WAVES = 4;          // waves (= pairs in flight) per workgroup
constexpr int PAIR_MAX_BLOCKS = 4096;  // beyond, a workgroup's waves loop over pairs

struct JacArgs {
    const float *z;
    const int64_t *nb;
    const float *other_table;
    int64_t other_rows;
    const float *own_table;
    const int64_t *owner;
    const float *W0, *b0, *w3, *b3, *fc;
    float *attn, *pooled_attn, *out, *D, *E, *dz;
    int64_t N;
    int R, L, F;
};

struct PairSide {                      // one side of a pair: the owner pass's outputs of that side's owners
    const float *p, *z, *attn, *E, *dz, *fc;
    float *glogit, *rev, *w;
    int R;
};

struct NarrePairArgs {
    PairSide user, item;
    const int64_t *u_idx, *i_idx;
    int64_t n_p;
    const float *q_bias, *c_bias, *W1, *b1, *w;
    int L, F;
    float *out_score, *g_user, *g_item;
};

struct NarrePairLds {                  // one wave's slice
    float x[NP_MAXL];                  // p_u o p_i
    float t[NP_MAXL];                  // W1 x + b1
    float up[NP_MAXL];                 // [t > 0] w
    float gx[NP_MAXL];                 // W1^T up
    float gu[NP_MAXL], gi[NP_MAXL];    // d score / d p_u, d score / d p_i
    float ga[NP_MAXR];                 // g . z_r
    float av[NP_MAXR];                 // a_r
    float dl[NP_MAXR];                 // delta_r
    float b[NP_MAXF];                  // g fc
};

__device__ __forceinline__ uint32_t np_lane_u32(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

// Sum over each 16-lane row, result in every lane of the row: wave_sum's four DPP steps.
__device__ __forceinline__ float np_row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xb1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4e, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));  // row_ror:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));  // row_ror:8
    return v;
}

// out[m] = sum_j W[m ld + j] v[j] (+ b[m]), m < nrows, j < ncols; v and out in the wave's LDS.  pair_grad.hip's
// rows_matvec: a 16-lane row per output, lane c chains j = c, c + 16, ..; every lane stays active.
__device__ __forceinline__ void np_rows_matvec(const float *__restrict__ W, int ld, int nrows, int ncols, const float *v,
                                               const float *__restrict__ b, float *out, int lane) {
    const int r = lane >> 4, c = lane & 15;
    for (int m0 = 0; m0 < nrows; m0 += 4) {
        const int m = m0 + r;
        const bool live = m < nrows;
        float acc = 0.f;
        if (live)
            for (int j = c; j < ncols; j += 16) acc = fmaf(W[(int64_t)m * ld + j], v[j], acc);
        acc = np_row16_sum(acc);
        if (live && c == 0) out[m] = b ? acc + b[m] : acc;
    }
}

// out[j] = sum_m v[m] W[m ld + j], j < ncols, m < nrows; v in the wave's LDS, out in LDS or global memory.
// pair_grad.hip's cols_matvec: lane = j (two filters per lane beyond 64 columns), m ascending in one chain.
__device__ __forceinline__ void np_cols_matvec(const float *__restrict__ W, int ld, int nrows, int ncols, const float *v,
                                               float *out, int lane) {
    for (int j = lane; j < ncols; j += WAVE) {
        float acc = 0.f;
#pragma unroll 4
        for (int m = 0; m < nrows; ++m) acc = fmaf(v[m], W[(int64_t)m * ld + j], acc);
        out[j] = acc;
    }
}

// LMAX: the class of L (L <= LMAX) -- it fixes the LDS strides, nothing of the arithmetic.
template <int LMAX>
__global__ __launch_bounds__(JAC_WAVES *WAVE) void narre_attn_jac_kernel(const JacArgs) {
    const JacArgs &a = kernel_args<JacArgs>();                 // each field an s_load next to its use (common.h)
    constexpr int CS = 2 * LMAX;       // floats per staged slot: [z_r ; other_r], zero padded
    constexpr int WS = 2 * LMAX + 4;   // floats per staged row of W0
    __shared__ __attribute__((aligned(16))) float w0s[LMAX * WS];
    __shared__ __attribute__((aligned(16))) float cats[JAC_WAVES][JAC_SLOTS * CS];
    const int R = a.R, L = a.L, F = a.F;
    const int C4 = (2 * L + 3) & ~3;   // the columns walked: 2L rounded up to the 16-byte reads, the pad holds zeros
    {
        const float *W0 = a.W0;
        for (int i = threadIdx.x; i < L * WS; i += JAC_WAVES * WAVE) {
            const int l = i / WS, c = i - l * WS;
            w0s[i] = c < 2 * L ? W0[(size_t)l * 2 * L + c] : 0.f;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    float *cat = cats[wave];
    const int lrow = lane < L ? lane : L - 1;                  // lanes past L walk a row that exists and count for nothing
    const float *wrow = w0s + lrow * WS;
    const float bias = a.b0[lrow];
    const float w3l = lane < L ? a.w3[lane] : 0.f;
    const float b3 = a.b3[0];
    const int64_t N = a.N, other_rows = a.other_rows;
    const float *other_table = a.other_table;
    for (int64_t n = (int64_t)blockIdx.x * JAC_WAVES + wave; n < N; n += (int64_t)gridDim.x * JAC_WAVES) {
        const float *zn = a.z + n * R * L;
        const int64_t *nbn = a.nb + n * R;
        float sc = -INFINITY;                                  // lane r: the logit of slot r
        uint32_t mlo = 0u, mhi = 0u;                           // lane r: the ReLU mask of slot r, bit m = [pre_rm > 0]
        for (int r0 = 0; r0 < R; r0 += JAC_SLOTS) {
            wave_lds_fence();                                  // the reads of the group (or owner) before are done
            for (int i = lane; i < JAC_SLOTS * CS; i += WAVE) {
                const int s = i / CS, c = i - s * CS, r = r0 + s;
                float v = 0.f;
                if (r < R) {
                    if (c < L) {
                        v = zn[r * L + c];
                    } else if (c < 2 * L) {
                        const int64_t id = nbn[r];
                        if (id >= 0 && id < other_rows) v = other_table[id * L + (c - L)];
                    }
                }
                cat[i] = v;
            }
            wave_lds_fence();
            float acc[JAC_SLOTS];
#pragma unroll
            for (int s = 0; s < JAC_SLOTS; ++s) acc[s] = 0.f;
            for (int c = 0; c < C4; c += 4) {
                const float4 w = *reinterpret_cast<const float4 *>(wrow + c);
#pragma unroll
                for (int s = 0; s < JAC_SLOTS; ++s) {
                    const float4 x = *reinterpret_cast<const float4 *>(cat + s * CS + c);
                    acc[s] = fmaf(w.x, x.x, acc[s]);
                    acc[s] = fmaf(w.y, x.y, acc[s]);
                    acc[s] = fmaf(w.z, x.z, acc[s]);
                    acc[s] = fmaf(w.w, x.w, acc[s]);
                }
            }
#pragma unroll
            for (int s = 0; s < JAC_SLOTS; ++s) {
                float h = acc[s] + bias;
                const uint64_t on = __builtin_amdgcn_ballot_w64(lane < L && h > 0.f);
                h = h > 0.f ? h : 0.f;
                const float t = wave_sum(w3l * h) + b3;
                if (lane == r0 + s) {
                    sc = t;
                    mlo = (uint32_t)on;
                    mhi = (uint32_t)(on >> 32);
                }
            }
        }
        if (lane >= R) sc = -INFINITY;
        const float m = wave_max(sc);
        const float e = lane < R ? expf(sc - m) : 0.f;
        const float den = wave_sum(e);
        const float w = e / den;                               // lane r: a_r; 0 in the lanes past R
        if (a.attn && lane < R) a.attn[n * R + lane] = w;
        if (a.out || a.pooled_attn) {
            float o = 0.f;
            const int l = lane < L ? lane : 0;
            for (int r = 0; r < R; ++r) o = fmaf(lane_value(w, r), zn[r * L + l], o);
            if (lane < L) {
                if (a.pooled_attn) a.pooled_attn[n * L + lane] = o;
                if (a.out) {
                    if (a.own_table) o += a.own_table[a.owner[n] * L + lane];
                    a.out[n * L + lane] = o;
                }
            }
        }
        if (a.D || a.E || a.dz) {
            float dzl = 0.f;                                   // lane r: dz_r
            for (int r = 0; r < R; ++r) {
                const uint32_t lo = np_lane_u32(mlo, r), hi = np_lane_u32(mhi, r);
                float d = 0.f;                                 // lane j: D_r[j], m ascending, a masked unit as 0.0f
                for (int mm = 0; mm < L; ++mm) {
                    const uint32_t bit = (mm < 32 ? lo >> mm : hi >> (mm - 32)) & 1u;
                    const float c = bit ? lane_value(w3l, mm) : 0.f;
                    d = fmaf(c, w0s[mm * WS + lrow], d);
                }
                const float zr = lane < L ? zn[r * L + lane] : 0.f;
                if (lane >= L) d = 0.f;
                if (a.D && lane < L) a.D[(n * R + r) * L + lane] = d;
                const float prod = d * zr;
                const float s = wave_sum(prod);
                if (lane == r) dzl = s;
                if (a.E) {
                    wave_lds_fence();                          // the reads of the slot before are done
                    if (lane < L) cat[lane] = d;
                    wave_lds_fence();
                    np_cols_matvec(a.fc, F, L, F, cat, a.E + (n * R + r) * F, lane);
                }
            }
            if (a.dz && lane < R) a.dz[n * R + lane] = dzl;
        }
    }
}

// One side of one pair: ga, dot, delta, rev and the [R, F] filter weights.  `o`: the side's owner row, `g` (LDS): the
// gradient with respect to that side's p.
__device__ __forceinline__ void narre_pair_side(const PairSide &s, int64_t o, int64_t p, int L, int F, const float *g,
                                                NarrePairLds &w, int lane) {
    if (!(s.glogit || s.rev || s.w)) return;
    const int R = s.R;
    np_rows_matvec(s.z + o * R * L, L, R, L, g, nullptr, w.ga, lane);      // ga_r = g . z_r
    if (lane < R) w.av[lane] = s.attn[o * R + lane];
    wave_lds_fence();
    float dot = 0.f;
    for (int r = 0; r < R; ++r) dot = fmaf(w.av[r], w.ga[r], dot);         // ascending r, the same chain in every lane
    const int rl = lane < R ? lane : 0;
    const float ar = w.av[rl], gar = w.ga[rl];
    const float dl = ar * (gar - dot);                                      // d score / d logit_r
    if (lane < R) {
        w.dl[lane] = dl;
        if (s.glogit) s.glogit[p * R + lane] = dl;
        if (s.rev) {
            const float direct = ar * gar;
            s.rev[p * R + lane] = fmaf(dl, s.dz[o * R + lane], direct);
        }
    }
    if (s.w) {
        np_cols_matvec(s.fc, F, L, F, g, w.b, lane);                        // b = g fc
        wave_lds_fence();
        const int RF = R * F;
        const float *E = s.E + o * RF;
        float *out = s.w + p * RF;
        for (int e = lane; e < RF; e += WAVE) {                             // the pair's [R, F] block, contiguous
            const int r = (int)((unsigned)e / (unsigned)F), f = e - r * F;
            const float direct = w.av[r] * w.b[f];
            out[e] = fmaf(w.dl[r], E[e], direct);
        }
    }
    wave_lds_fence();                                                       // the reads of this side are done
}

__global__ __launch_bounds__(PAIR_WAVES *WAVE) void narre_pair_grad_kernel(const NarrePairArgs) {
    const NarrePairArgs &a = kernel_args<NarrePairArgs>();     // each field an s_load next to its use (common.h)
    __shared__ __attribute__((aligned(16))) NarrePairLds lds[PAIR_WAVES];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    NarrePairLds &w = lds[wave];
    const int L = a.L, F = a.F;
    const int64_t n_p = a.n_p;
    for (int64_t p = (int64_t)blockIdx.x * PAIR_WAVES + wave; p < n_p; p += (int64_t)gridDim.x * PAIR_WAVES) {
        const int64_t u = a.u_idx[p], i = a.i_idx[p];
        wave_lds_fence();                                      // the reads of the pair before are done
        float pu = 0.f, pi = 0.f;
        if (lane < L) {
            pu = a.user.p[u * L + lane];
            pi = a.item.p[i * L + lane];
            w.x[lane] = pu * pi;
        }
        wave_lds_fence();
        np_rows_matvec(a.W1, L, L, L, w.x, a.b1, w.t, lane);   // t = W1 x + b1
        wave_lds_fence();
        float term = 0.f;
        if (lane < L) {
            const float tm = w.t[lane], wm = a.w[lane];
            term = wm * fmaxf(tm, 0.f);
            w.up[lane] = tm > 0.f ? wm : 0.f;                  // the upstream of t: [t > 0] w
        }
        const float head = wave_sum(term);
        wave_lds_fence();
        np_cols_matvec(a.W1, L, L, L, w.up, w.gx, lane);       // gx = W1^T ([t > 0] w)
        wave_lds_fence();
        if (lane < L) {
            const float gx = w.gx[lane];
            const float gu = gx * pi, gi = gx * pu;
            w.gu[lane] = gu;
            w.gi[lane] = gi;
            if (a.g_user) a.g_user[p * L + lane] = gu;
            if (a.g_item) a.g_item[p * L + lane] = gi;
        }
        wave_lds_fence();
        if (lane == 0 && a.out_score) {
            const float qb = a.q_bias ? a.q_bias[u] : 0.f, cb = a.c_bias ? a.c_bias[i] : 0.f;
            a.out_score[p] = (head + qb) + cb;
        }
        narre_pair_side(a.user, u, p, L, F, w.gu, w, lane);
        narre_pair_side(a.item, i, p, L, F, w.gi, w, lane);
    }
}

}  // namespace r4r

using namespace r4r;

extern "C" int r4r_narre_attn_jac(const float *z, const int64_t *nb, const float *other_table, int64_t other_rows,
                                  const float *own_table, const int64_t *owner, const float *W0, const float *b0,
                                  const float *w3, const float *b3, const float *fc, int F, float *attn,
                                  float *pooled_attn, float *out, float *D, float *E, float *dz, int64_t N, int R, int L,
                                  void *stream) {
    R4R_REQUIRE(N >= 0 && other_rows >= 0, "r4r_narre_attn_jac: negative size (N=%lld other_rows=%lld)", (long long)N,
                (long long)other_rows);
    R4R_REQUIRE(R >= 1 && R <= NP_MAXR, "r4r_narre_attn_jac: R=%d reviews outside 1..%d", R, NP_MAXR);
    R4R_REQUIRE(L >= 1 && L <= NP_MAXL, "r4r_narre_attn_jac: L=%d latent units outside 1..%d", L, NP_MAXL);
    R4R_REQUIRE(F >= 1 && F <= NP_MAXF, "r4r_narre_attn_jac: F=%d filters outside 1..%d", F, NP_MAXF);
    R4R_REQUIRE((own_table == nullptr) == (owner == nullptr), "r4r_narre_attn_jac: own_table and owner go together");
    R4R_REQUIRE(!E || fc, "r4r_narre_attn_jac: E without fc (null pointer)");
    if (N == 0) return R4R_OK;
    R4R_REQUIRE(z && nb && W0 && b0 && w3 && b3, "r4r_narre_attn_jac: null pointer among z, nb, W0, b0, w3, b3");
    R4R_REQUIRE(other_table || other_rows == 0, "r4r_narre_attn_jac: null other_table with other_rows=%lld",
                (long long)other_rows);
    R4R_REQUIRE(attn || pooled_attn || out || D || E || dz, "r4r_narre_attn_jac: no output asked for (all six are null)");
    JacArgs a{z, nb, other_table, other_rows, own_table, owner, W0, b0, w3, b3, fc, attn, pooled_attn, out, D, E, dz,
              N, R, L, F};
    const int64_t want = cdiv(N, JAC_WAVES);
    const dim3 grid((unsigned)(want < JAC_MAX_BLOCKS ? want : JAC_MAX_BLOCKS)), block(JAC_WAVES * WAVE);
    hipStream_t st = as_stream(stream);
    if (L <= 16)
        hipLaunchKernelGGL(narre_attn_jac_kernel<16>, grid, block, 0, st, a);
    else if (L <= 32)
        hipLaunchKernelGGL(narre_attn_jac_kernel<32>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(narre_attn_jac_kernel<64>, grid, block, 0, st, a);
    return check_launch("r4r_narre_attn_jac");
}

extern "C" int r4r_narre_pair_grad(const float *p_u, const float *z_u, const float *attn_u, const float *E_u,
                                   const float *dz_u, const float *fc_u, int64_t n_u, int R_u, const float *p_i,
                                   const float *z_i, const float *attn_i, const float *E_i, const float *dz_i,
                                   const float *fc_i, int64_t n_i, int R_i, const int64_t *u_idx, const int64_t *i_idx,
                                   int64_t n_p, const float *q_bias, const float *c_bias, const float *W1, const float *b1,
                                   const float *w, int L, int F, float *out_score, float *g_user, float *g_item,
                                   float *glogit_user, float *glogit_item, float *rev_user, float *rev_item, float *w_user,
                                   float *w_item, void *stream) {
    R4R_REQUIRE(R_u >= 1 && R_u <= NP_MAXR, "r4r_narre_pair_grad: R_u=%d reviews outside 1..%d", R_u, NP_MAXR);
    R4R_REQUIRE(R_i >= 1 && R_i <= NP_MAXR, "r4r_narre_pair_grad: R_i=%d reviews outside 1..%d", R_i, NP_MAXR);
    R4R_REQUIRE(L >= 1 && L <= NP_MAXL, "r4r_narre_pair_grad: L=%d latent units outside 1..%d", L, NP_MAXL);
    R4R_REQUIRE(F >= 1 && F <= NP_MAXF, "r4r_narre_pair_grad: F=%d filters outside 1..%d", F, NP_MAXF);
    R4R_REQUIRE(n_u >= 0 && n_i >= 0, "r4r_narre_pair_grad: n_u=%lld / n_i=%lld negative", (long long)n_u, (long long)n_i);
    R4R_REQUIRE(n_p >= 0 && n_p < (1ll << 31), "r4r_narre_pair_grad: n_p=%lld pairs outside 0..2^31-1", (long long)n_p);
    R4R_REQUIRE(!w_user || fc_u, "r4r_narre_pair_grad: w_user without fc_u (null pointer)");
    R4R_REQUIRE(!w_item || fc_i, "r4r_narre_pair_grad: w_item without fc_i (null pointer)");
    R4R_REQUIRE(!w_user || E_u, "r4r_narre_pair_grad: w_user without E_u (null pointer)");
    R4R_REQUIRE(!w_item || E_i, "r4r_narre_pair_grad: w_item without E_i (null pointer)");
    R4R_REQUIRE(!rev_user || dz_u, "r4r_narre_pair_grad: rev_user without dz_u (null pointer)");
    R4R_REQUIRE(!rev_item || dz_i, "r4r_narre_pair_grad: rev_item without dz_i (null pointer)");
    R4R_REQUIRE(!(glogit_user || rev_user || w_user) || (z_u && attn_u),
                "r4r_narre_pair_grad: glogit_user / rev_user / w_user without z_u and attn_u (null pointer)");
    R4R_REQUIRE(!(glogit_item || rev_item || w_item) || (z_i && attn_i),
                "r4r_narre_pair_grad: glogit_item / rev_item / w_item without z_i and attn_i (null pointer)");
    if (n_p == 0) return R4R_OK;
    R4R_REQUIRE(p_u && p_i && u_idx && i_idx, "r4r_narre_pair_grad: null pointer among p_u, p_i, u_idx, i_idx");
    R4R_REQUIRE(W1 && b1 && w, "r4r_narre_pair_grad: null pointer among W1, b1, w");
    R4R_REQUIRE(n_u >= 1 && n_i >= 1, "r4r_narre_pair_grad: n_p=%lld pairs over n_u=%lld / n_i=%lld rows", (long long)n_p,
                (long long)n_u, (long long)n_i);
    NarrePairArgs a{{p_u, z_u, attn_u, E_u, dz_u, fc_u, glogit_user, rev_user, w_user, R_u},
                    {p_i, z_i, attn_i, E_i, dz_i, fc_i, glogit_item, rev_item, w_item, R_i},
                    u_idx, i_idx, n_p, q_bias, c_bias, W1, b1, w, L, F, out_score, g_user, g_item};
    const int64_t want = cdiv(n_p, PAIR_WAVES);
    const dim3 grid((unsigned)(want < PAIR_MAX_BLOCKS ? want : PAIR_MAX_BLOCKS)), block(PAIR_WAVES * WAVE);
    hipLaunchKernelGGL(narre_pair_grad_kernel, grid, block, 0, as_stream(stream), a);
    return check_launch("r4r_narre_pair_grad");
}

// Pair gradients for gfx950 (include/r4r.h, "Pair gradients"): for explicit (user, item) pairs over the eval-mode tower
// latents zu [n_u, L] and zi [n_i, L], the model's prediction, its gradient with respect to both latents and that
// gradient carried back through each tower's fc to the F pooled features -- the per-row filter weights
// r4r_textcnn_phrases takes.  One launch, the model's RAW head parameters.
//
// Reference behaviour restated (dropout is the identity in eval mode, common_pytorch_models.py:37):
//   fm    deepconn      DeepCoNN.py:61-66, TorchFM common_pytorch_models.py:49-57 over x = [zu ; zi]
//   mlp   deepconn++    DeepCoNN.py:68-72: Linear(2L, L) -> ReLU -> Linear(L, 1)
//   pfm   transnet(++)  TransNet.py:25-35 (Linear -> ReLU -> Linear) and 105-114 (source_fm over [eu ; ei ; ir])
//
// One WAVE per pair, PG_WAVES independent waves per workgroup (no workgroup barrier at all), grid-strided.  A wave keeps
// its pair's vectors (x, a, h, y, the gradients) in its own LDS slice and hands them from step to step through
// wave_lds_fence.  The matrices are read from global memory in two shapes only:
//   rows_matvec  out[m] = sum_j W[m, j] v[j] + b[m]: a 16-lane row per output, lane c of the row takes j = c, c + 16, ..
//                ascending in one fmaf chain from 0.0f (64 contiguous bytes per row and load), the 16 partials are summed
//                by four DPP steps (xor 1, xor 2, ror 4, ror 8), then + b[m].  Four outputs per pass.
//   cols_matvec  out[j] = sum_m v[m] W[m, j]: lane = j (j, j + 64, .. beyond 64 columns: two filters per lane for F > 64),
//                m ascending in one fmaf chain from 0.0f; v[m] is an LDS broadcast, W[m, .] a coalesced row.  No reduction.
// The head's matrices and both fc (at most 106 KiB at L = 64, F = 112) are NOT staged in LDS: every wave of a launch
// reads the same few rows, which L2 (4 MiB) and the CU's vector cache serve, and a workgroup of four pairs would read
// all of them once to use each element four times.  DESIGN 4.24 has the reasoning and what was measured.
// A pair's outputs depend on that pair's inputs only: not on n_p, the grid, the other pairs, or which outputs are NULL
// (every wave runs the same instruction sequence up to the stores; only the two back-projections are skipped as a
// whole when their output is NULL).
#include "common.h"

namespace r4r {

constexpr int PG_WAVES = 4;            // waves (= pairs in flight) per workgroup
constexpr int PG_MAX_BLOCKS = 4096;    // beyond, a workgroup's waves loop over pairs
constexpr int PG_RANK = 8;             // TorchFM's k (DeepCoNN.py:32, TransNet.py:77-79)
constexpr int PG_FM_MAXL = 128, PG_MLP_MAXL = 64, PG_MAXP = 8, PG_MAXF = 112;
constexpr int PG_MAXX = 2 * PG_FM_MAXL;               // x = [zu ; zi]
constexpr int PG_MAXY = 2 * PG_MAXP + PG_MLP_MAXL;    // y = [eu ; ei ; ir]

struct PairGradArgs {
    const float *zu, *zi;
    const int64_t *u_idx, *i_idx;
    int64_t n_p;
    const float *q_bias, *c_bias;
    const float *W0, *b0, *W2, *b2, *w3, *V, *lw, *xu, *xi, *fc_u, *fc_i;
    int P, L, F;
    float *out_score, *g_user, *g_item, *w_user, *w_item;
};

struct PairGradLds {                   // one wave's slice
    float x[PG_MAXX];                  // [zu ; zi]
    float g[PG_MAXX];                  // d score / d x
    float y[PG_MAXY];                  // pfm: [eu ; ei ; ir]
    float gy[PG_MAXY];                 // pfm: d score / d y
    float a[PG_MLP_MAXL];              // W0 x + b0
    float h[PG_MLP_MAXL];              // relu(a); then the masked upstream of a
    float t[PG_MLP_MAXL];              // pfm: W2^T gy[2P:]
    float part[WAVE];                  // the FM's 8 x 8 partial sums
    float s[PG_RANK];                  // the FM's s_k
};

// Sum over each 16-lane row, result in every lane of the row: wave_sum's four DPP steps.
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xb1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4e, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));  // row_ror:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));  // row_ror:8
    return v;
}

// out[m] = sum_j W[m ld + j] v[j] + b[m], m < nrows, j < ncols; v and out in the wave's LDS.  Every lane stays active.
__device__ __forceinline__ void rows_matvec(const float *__restrict__ W, int ld, int nrows, int ncols, const float *v,
                                            const float *__restrict__ b, float *out, int lane) {
    const int r = lane >> 4, c = lane & 15;
    for (int m0 = 0; m0 < nrows; m0 += 4) {
        const int m = m0 + r;
        const bool live = m < nrows;
        float acc = 0.f;
        if (live)
            for (int j = c; j < ncols; j += 16) acc = fmaf(W[(int64_t)m * ld + j], v[j], acc);
        acc = row16_sum(acc);
        if (live && c == 0) out[m] = acc + b[m];
    }
}

// out[j] = sum_m v[m] W[m ld + j], j < ncols, m < nrows; v in the wave's LDS, out in LDS or global memory.
__device__ __forceinline__ void cols_matvec(const float *__restrict__ W, int ld, int nrows, int ncols, const float *v,
                                            float *out, int lane) {
    for (int j = lane; j < ncols; j += WAVE) {
        float acc = 0.f;
#pragma unroll 4
        for (int m = 0; m < nrows; ++m) acc = fmaf(v[m], W[(int64_t)m * ld + j], acc);
        out[j] = acc;
    }
}

// TorchFM over y [n] (the wave's LDS) without its bias: returns lin + 1/2 (sum_k s_k^2 - sum_j y_j^2 sum_k V_jk^2) in
// every lane and writes gy[j] = lw_j + sum_k s_k V_jk - y_j sum_k V_jk^2.
__device__ __forceinline__ float fm_head(const float *__restrict__ V, const float *__restrict__ lw, int n, const float *y,
                                         float *gy, PairGradLds &w, int lane) {
    {   // s_k: lane (jg, k) sums j = jg, jg + 8, .. ascending; lane k < 8 then adds the 8 partials in ascending jg
        const int jg = lane >> 3, k = lane & 7;
        float acc = 0.f;
        for (int j = jg; j < n; j += 8) acc = fmaf(y[j], V[j * PG_RANK + k], acc);
        w.part[lane] = acc;
        wave_lds_fence();
        if (lane < PG_RANK) {
            float s = w.part[lane];
#pragma unroll
            for (int g = 1; g < 8; ++g) s += w.part[g * 8 + lane];
            w.s[lane] = s;
        }
        wave_lds_fence();
    }
    float s[PG_RANK];
#pragma unroll
    for (int k = 0; k < PG_RANK; ++k) s[k] = w.s[k];
    float lin = 0.f, q2 = 0.f;
    for (int j = lane; j < n; j += WAVE) {
        const float yj = y[j], lj = lw[j];
        float v2 = 0.f, dot = 0.f;
#pragma unroll
        for (int k = 0; k < PG_RANK; ++k) {
            const float v = V[j * PG_RANK + k];
            v2 = fmaf(v, v, v2);
            dot = fmaf(s[k], v, dot);
        }
        gy[j] = fmaf(-yj, v2, lj + dot);
        lin = fmaf(lj, yj, lin);
        q2 = fmaf(yj * yj, v2, q2);
    }
    lin = wave_sum(lin);
    q2 = wave_sum(q2);
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < PG_RANK; ++k) ss = fmaf(s[k], s[k], ss);
    wave_lds_fence();                                          // gy is written
    return fmaf(0.5f, ss - q2, lin);
}

template <int KIND>
__global__ __launch_bounds__(PG_WAVES *WAVE) void pair_grad_kernel(const PairGradArgs) {
    const PairGradArgs &a = kernel_args<PairGradArgs>();      // each field an s_load next to its use (common.h)
    __shared__ __attribute__((aligned(16))) PairGradLds lds[PG_WAVES];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    PairGradLds &w = lds[wave];
    const int L = a.L, F = a.F, P = a.P, X = 2 * L;
    for (int64_t p = (int64_t)blockIdx.x * PG_WAVES + wave; p < a.n_p; p += (int64_t)gridDim.x * PG_WAVES) {
        const int64_t u = a.u_idx[p], i = a.i_idx[p];
        wave_lds_fence();                                      // the reads of the pair before are done
        for (int j = lane; j < X; j += WAVE) w.x[j] = j < L ? a.zu[u * L + j] : a.zi[i * L + (j - L)];
        wave_lds_fence();
        float score;
        if constexpr (KIND == R4R_PAIR_GRAD_FM) {
            score = fm_head(a.V, a.lw, X, w.x, w.g, w, lane);
        } else {
            rows_matvec(a.W0, X, L, X, w.x, a.b0, w.a, lane);  // a = W0 x + b0
            wave_lds_fence();
            if constexpr (KIND == R4R_PAIR_GRAD_MLP) {
                float term = 0.f;
                if (lane < L) {
                    const float am = w.a[lane], w3 = a.w3[lane];
                    term = w3 * fmaxf(am, 0.f);
                    w.h[lane] = am > 0.f ? w3 : 0.f;           // the upstream of a: [a > 0] w3
                }
                score = wave_sum(term);
                wave_lds_fence();
            } else {
                if (lane < L) w.h[lane] = fmaxf(w.a[lane], 0.f);
                for (int f = lane; f < 2 * P; f += WAVE) w.y[f] = f < P ? a.xu[u * P + f] : a.xi[i * P + (f - P)];
                wave_lds_fence();
                rows_matvec(a.W2, L, L, L, w.h, a.b2, w.y + 2 * P, lane);      // ir = W2 relu(a) + b2
                wave_lds_fence();
                score = fm_head(a.V, a.lw, 2 * P + L, w.y, w.gy, w, lane);
                cols_matvec(a.W2, L, L, L, w.gy + 2 * P, w.t, lane);           // t = W2^T gy[2P:]
                wave_lds_fence();
                if (lane < L) w.h[lane] = w.a[lane] > 0.f ? w.t[lane] : 0.f;   // the upstream of a: [a > 0] t
                wave_lds_fence();
            }
            cols_matvec(a.W0, X, L, X, w.h, w.g, lane);        // g = W0^T ([a > 0] upstream)
            wave_lds_fence();
        }
        if (lane == 0 && a.out_score) {
            const float qb = a.q_bias ? a.q_bias[u] : 0.f, cb = a.c_bias ? a.c_bias[i] : 0.f;
            a.out_score[p] = (score + qb) + cb;
        }
        for (int j = lane; j < L; j += WAVE) {
            if (a.g_user) a.g_user[p * L + j] = w.g[j];
            if (a.g_item) a.g_item[p * L + j] = w.g[L + j];
        }
        if (a.w_user) cols_matvec(a.fc_u, F, L, F, w.g, a.w_user + p * F, lane);       // w = g fc: lane = filter
        if (a.w_item) cols_matvec(a.fc_i, F, L, F, w.g + L, a.w_item + p * F, lane);
    }
}

}  // namespace r4r

using namespace r4r;

extern "C" int r4r_pair_grad(int kind, const float *zu, int64_t n_u, const float *zi, int64_t n_i, const int64_t *u_idx,
                             const int64_t *i_idx, int64_t n_p, const float *q_bias, const float *c_bias,
                             const float *W0, const float *b0, const float *W2, const float *b2, const float *w3,
                             const float *V, const float *lw, const float *xu, const float *xi, int P,
                             const float *fc_u, const float *fc_i, int L, int F, float *out_score, float *g_user,
                             float *g_item, float *w_user, float *w_item, void *stream) {
    R4R_REQUIRE(kind == R4R_PAIR_GRAD_FM || kind == R4R_PAIR_GRAD_MLP || kind == R4R_PAIR_GRAD_PFM,
                "r4r_pair_grad: kind=%d is none of fm (0), mlp (1), pfm (2)", kind);
    const int max_l = kind == R4R_PAIR_GRAD_FM ? PG_FM_MAXL : PG_MLP_MAXL;
    R4R_REQUIRE(L >= 1 && L <= max_l, "r4r_pair_grad: L=%d outside 1..%d for kind %d", L, max_l, kind);
    R4R_REQUIRE(F >= 1 && F <= PG_MAXF, "r4r_pair_grad: F=%d filters outside 1..%d", F, PG_MAXF);
    R4R_REQUIRE(P >= 0 && P <= PG_MAXP, "r4r_pair_grad: P=%d outside 0..%d", P, PG_MAXP);
    R4R_REQUIRE(kind == R4R_PAIR_GRAD_PFM || P == 0, "r4r_pair_grad: P=%d id-embedding columns, but only pfm has them", P);
    R4R_REQUIRE(n_u >= 0 && n_i >= 0, "r4r_pair_grad: n_u=%lld / n_i=%lld negative", (long long)n_u, (long long)n_i);
    R4R_REQUIRE(n_p >= 0 && n_p < (1ll << 31), "r4r_pair_grad: n_p=%lld pairs outside 0..2^31-1", (long long)n_p);
    if (kind == R4R_PAIR_GRAD_FM) R4R_REQUIRE(V && lw, "r4r_pair_grad: fm needs V and lw, got a null pointer");
    if (kind == R4R_PAIR_GRAD_MLP) R4R_REQUIRE(W0 && b0 && w3, "r4r_pair_grad: mlp needs W0, b0 and w3, got a null pointer");
    if (kind == R4R_PAIR_GRAD_PFM) {
        R4R_REQUIRE(W0 && b0 && W2 && b2 && V && lw, "r4r_pair_grad: pfm needs W0, b0, W2, b2, V and lw, got a null pointer");
        R4R_REQUIRE(P == 0 || (xu && xi), "r4r_pair_grad: P=%d needs the id-embedding tables xu and xi, got a null pointer", P);
    }
    R4R_REQUIRE(!w_user || fc_u, "r4r_pair_grad: w_user without fc_u (null pointer)");
    R4R_REQUIRE(!w_item || fc_i, "r4r_pair_grad: w_item without fc_i (null pointer)");
    if (n_p == 0) return R4R_OK;
    R4R_REQUIRE(zu && zi && u_idx && i_idx, "r4r_pair_grad: null pointer among zu, zi, u_idx, i_idx");
    R4R_REQUIRE(n_u >= 1 && n_i >= 1, "r4r_pair_grad: n_p=%lld pairs over n_u=%lld / n_i=%lld rows", (long long)n_p,
                (long long)n_u, (long long)n_i);
    PairGradArgs a{zu, zi, u_idx, i_idx, n_p, q_bias, c_bias, W0, b0, W2, b2, w3, V, lw, xu, xi, fc_u, fc_i,
                   P, L, F, out_score, g_user, g_item, w_user, w_item};
    const int64_t want = cdiv(n_p, PG_WAVES);
    const dim3 grid((unsigned)(want < PG_MAX_BLOCKS ? want : PG_MAX_BLOCKS)), block(PG_WAVES * WAVE);
    hipStream_t st = as_stream(stream);
    if (kind == R4R_PAIR_GRAD_FM)
        hipLaunchKernelGGL(pair_grad_kernel<R4R_PAIR_GRAD_FM>, grid, block, 0, st, a);
    else if (kind == R4R_PAIR_GRAD_MLP)
        hipLaunchKernelGGL(pair_grad_kernel<R4R_PAIR_GRAD_MLP>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(pair_grad_kernel<R4R_PAIR_GRAD_PFM>, grid, block, 0, st, a);
    return check_launch("r4r_pair_grad");
}

// Phrase explanations for gfx950 (include/r4r.h, "Phrase explanations"): the word windows that win a TextCNN tower's
// max-pool, listed per row from what r4r_textcnn_fwd already returns -- pooled [N, F] and argmax [N, F].
//
// Reference behaviour restated: the tower of common_pytorch_models.py:29-31 is conv 3 x E (pad 2) -> ReLU -> global
// max-pool, so filter f of a document contributes the activation of ONE three-word window, the one at argmax[n, f], and
// the latent vector (DeepCoNN.py:53-54, NARRE.py:95-96, TransNet.py:100-102) is a linear image of those F numbers.  A
// row's windows are grouped by position, scored by the (weighted) sum of the pooled values they won and listed by score.
//
// One WAVE per row, PH_WAVES independent waves per workgroup (no workgroup barrier at all), grid-strided.  Per row:
//   1. lane l stages filters l and l + 64 in the wave's own LDS: position (-1 for a dead filter), pooled value, weight
//      (1.0f without weights: fmaf(1, p, acc) is acc + p, bit for bit).
//   2. every filter walks the staged filters in ascending f, 4 per 16-byte broadcast read: it is the LEADER of its window
//      iff no lower filter has its position, and it sums its window's fmaf chain in that order.  Every member of a window
//      runs the same chain; only the leader's result is kept.
//   3. the leaders' (position, score) go back to LDS; a leader's place is the count of leaders ahead of it (score
//      descending, ties by ascending position -- positions are distinct, so the order is total), and below K it stores
//      itself AT its place.  Places min(K, windows) .. K get the fill.
// No sort, no atomics, no MFMA: 2 F^2 / 64 compares per lane and the row's 8 F bytes.  A row's outputs depend on that
// row's inputs only: not on N, the grid, K, or which outputs are asked for.
#include "common.h"

namespace r4r {

constexpr int PH_MAXF = 112;           // r4r_textcnn_fwd's limit
constexpr int PH_SLOTS = 128;          // staged filters per wave: two per lane
#ifndef R4R_PH_WAVES
#define R4R_PH_WAVES 4
#endif
constexpr int PH_WAVES = R4R_PH_WAVES; // waves (= rows in flight) per workgroup
constexpr int PH_MAX_BLOCKS = 4096;    // beyond, a workgroup's waves loop over rows

struct PhrasesArgs {
    const float *pooled;
    const int32_t *argmax;
    const float *wt;
    int64_t wt_stride;
    const int64_t *idx;
    int64_t N;
    int T, F, K;
    int32_t *top_pos;
    float *top_score;
    int32_t *top_filters;
    int64_t *top_tok;
    int32_t *n_windows;
};

__global__ __launch_bounds__(PH_WAVES *WAVE) void textcnn_phrases_kernel(const PhrasesArgs a) {
    __shared__ __attribute__((aligned(16))) int spos[PH_WAVES][PH_SLOTS];
    __shared__ __attribute__((aligned(16))) float sval[PH_WAVES][PH_SLOTS];
    __shared__ __attribute__((aligned(16))) float swt[PH_WAVES][PH_SLOTS];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    int *pos = spos[wave];
    float *val = sval[wave], *wgt = swt[wave];
    const int F = a.F, T = a.T, K = a.K;
    const int F4 = (F + 3) & ~3;                               // the filters walked: the pad holds dead ones
    const int halves = F > WAVE ? 2 : 1;                       // wave-uniform: lanes hold a second filter only past 64
    for (int64_t n = (int64_t)blockIdx.x * PH_WAVES + wave; n < a.N; n += (int64_t)gridDim.x * PH_WAVES) {
        // ---- 1. stage
        int my_pos[2];
        wave_lds_fence();                                      // the reads of the row before are done
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int f = lane + h * WAVE;
            int p = -1;
            float v = 0.f, w = 0.f;
            if (f < F) {
                const int am = a.argmax[n * F + f];
                p = (am >= 0 && am < T + 2) ? am : -1;
                v = a.pooled[n * F + f];
                w = a.wt ? a.wt[n * a.wt_stride + f] : 1.f;
            }
            my_pos[h] = p;
            pos[f] = p;
            val[f] = v;
            wgt[f] = w;
        }
        wave_lds_fence();
        // ---- 2. leaders and their windows' sums, ascending f
        float score[2] = {0.f, 0.f};
        int count[2] = {0, 0};
        bool lead[2] = {false, false};
        for (int h = 0; h < halves; ++h) {
            const int f = lane + h * WAVE, mp = my_pos[h];
            float acc = 0.f;
            int cnt = 0, lower = 0;
            for (int g = 0; g < F4; g += 4) {
                const int4 gp = *reinterpret_cast<const int4 *>(pos + g);
                const float4 gv = *reinterpret_cast<const float4 *>(val + g);
                const float4 gw = *reinterpret_cast<const float4 *>(wgt + g);
                const bool e0 = gp.x == mp, e1 = gp.y == mp, e2 = gp.z == mp, e3 = gp.w == mp;
                acc = e0 ? fmaf(gw.x, gv.x, acc) : acc;
                acc = e1 ? fmaf(gw.y, gv.y, acc) : acc;
                acc = e2 ? fmaf(gw.z, gv.z, acc) : acc;
                acc = e3 ? fmaf(gw.w, gv.w, acc) : acc;
                cnt += (int)e0 + (int)e1 + (int)e2 + (int)e3;
                lower += (int)(e0 && g < f) + (int)(e1 && g + 1 < f) + (int)(e2 && g + 2 < f) + (int)(e3 && g + 3 < f);
            }
            lead[h] = mp >= 0 && lower == 0;
            score[h] = acc;
            count[h] = cnt;
        }
        const int windows = __popcll(__ballot(lead[0])) + __popcll(__ballot(lead[1]));
        // ---- 3. the leaders back to LDS (-1: not a leader), then places
        wave_lds_fence();                                      // every lane's walk over pos / val is done
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int f = lane + h * WAVE;
            pos[f] = lead[h] ? my_pos[h] : -1;
            val[f] = score[h];
        }
        wave_lds_fence();
        for (int h = 0; h < halves; ++h) {
            if (!lead[h]) continue;                            // (divergent from here on: plain loads and stores only)
            const int mp = my_pos[h];
            const float ms = score[h];
            int place = 0;
            for (int g = 0; g < F4; g += 4) {
                const int4 gp = *reinterpret_cast<const int4 *>(pos + g);
                const float4 gv = *reinterpret_cast<const float4 *>(val + g);
                place += (int)(gp.x >= 0 && (gv.x > ms || (gv.x == ms && gp.x < mp)));
                place += (int)(gp.y >= 0 && (gv.y > ms || (gv.y == ms && gp.y < mp)));
                place += (int)(gp.z >= 0 && (gv.z > ms || (gv.z == ms && gp.z < mp)));
                place += (int)(gp.w >= 0 && (gv.w > ms || (gv.w == ms && gp.w < mp)));
            }
            if (place < K) {
                const int64_t at = n * K + place;
                if (a.top_pos) a.top_pos[at] = mp;
                if (a.top_score) a.top_score[at] = ms;
                if (a.top_filters) a.top_filters[at] = count[h];
                if (a.top_tok) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const int t = mp - 2 + j;
                        a.top_tok[at * 3 + j] = (t >= 0 && t < T) ? a.idx[n * T + t] : -1;
                    }
                }
            }
        }
        for (int e = windows + lane; e < K; e += WAVE) {       // the places beyond min(K, windows)
            const int64_t at = n * K + e;
            if (a.top_pos) a.top_pos[at] = -1;
            if (a.top_score) a.top_score[at] = 0.f;
            if (a.top_filters) a.top_filters[at] = 0;
            if (a.top_tok) a.top_tok[at * 3] = a.top_tok[at * 3 + 1] = a.top_tok[at * 3 + 2] = -1;
        }
        if (a.n_windows && lane == 0) a.n_windows[n] = windows;
    }
}

}  // namespace r4r

using namespace r4r;

extern "C" int r4r_textcnn_phrases(const float *pooled, const int32_t *argmax, const float *wt, int64_t wt_stride,
                                   const int64_t *idx, int64_t N, int T, int F, int K, int32_t *top_pos,
                                   float *top_score, int32_t *top_filters, int64_t *top_tok, int32_t *n_windows,
                                   void *stream) {
    R4R_REQUIRE(pooled && argmax, "r4r_textcnn_phrases: null pooled / argmax");
    R4R_REQUIRE(F >= 1 && F <= PH_MAXF, "r4r_textcnn_phrases: F=%d filters outside 1..%d", F, PH_MAXF);
    R4R_REQUIRE(K >= 1 && K <= F, "r4r_textcnn_phrases: K=%d outside 1..F=%d", K, F);
    R4R_REQUIRE(T >= 1, "r4r_textcnn_phrases: T=%d words, at least 1", T);
    R4R_REQUIRE(N >= 0 && N < (1ll << 31), "r4r_textcnn_phrases: N=%lld rows outside 0..2^31-1", (long long)N);
    R4R_REQUIRE(wt_stride == 0 || wt_stride == F, "r4r_textcnn_phrases: wt_stride=%lld is neither 0 nor F=%d",
                (long long)wt_stride, F);
    R4R_REQUIRE(!top_tok || idx, "r4r_textcnn_phrases: top_tok without idx (the documents)");
    if (N == 0) return R4R_OK;
    PhrasesArgs a{pooled, argmax, wt, wt_stride, idx, N, T, F, K, top_pos, top_score, top_filters, top_tok, n_windows};
    const int64_t want = cdiv(N, PH_WAVES);
    const unsigned blocks = (unsigned)(want < PH_MAX_BLOCKS ? want : PH_MAX_BLOCKS);
    hipLaunchKernelGGL(textcnn_phrases_kernel, dim3(blocks), dim3(PH_WAVES * WAVE), 0, as_stream(stream), a);
    return check_launch("r4r_textcnn_phrases");
}

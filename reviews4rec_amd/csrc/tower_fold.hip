// Document fold for gfx950 (include/r4r.h, "Document fold"): the pooled features of a VARIANT of an owner's document --
// chosen reviews taken away -- without building the document and without the tower's gather.
//
// Reference behaviour restated: the tower of common_pytorch_models.py:29-31 is conv 3 x E (pad 2) -> ReLU -> global
// max-pool over the document of data.py:223-235 (the owner's reviews joined, cut to input_length, padded with word 0),
// and DeepCoNN.py:53-54 looks the words up in a frozen table.  With ptab[v, j, :] = table[v] . conv_w[:, j, :] a window
// over the tokens (a, c, d) is ((ptab[a, 0] + ptab[c, 1]) + ptab[d, 2]) + conv_b: three rows and nothing else, so a
// window that lies inside one review keeps its bits wherever a removal shifts that review.  Per (owner, review) the
// maximum over those interior windows is cached once (`seg`); a variant row then needs the two windows at each kept
// review's first words, the review cut by T, the tail beyond the 64th review, the padding and the two windows hanging
// over the end.
//
//   fold_project_kernel   ptab = table x conv_w^T, a 64 x 64 tile per workgroup, 4 x 4 per thread, fmaf chains in
//                         ascending k.
//   fold_segments_kernel  one wave per (owner, review): the review's tokens 64 at a time, one per lane, then lanes are
//                         filters (two per lane, as in phrases.hip) and every window is three row reads.
//   fold_compose_kernel   one wave per row: lanes are review slots for the kept lengths, their running sum
//                         (docs_masked_device.h's scan) and each kept review's first / last two tokens -- all requested
//                         together; the windows' token triples go to the wave's LDS, then lanes are filters.
//   fold_search_*_kernel  the search's bookkeeping: the start state, a step's candidate rows out of the pairs' masks,
//                         and the winner of a step's scores.  Integer work and one latent row copied per pair.
// No workgroup barrier outside the GEMM, no atomics; a row's outputs depend on that row's inputs only.
#include <math.h>

#include "common.h"

namespace r4r {

constexpr int FD_MAXF = 112;                 // r4r_textcnn_fwd's limit
constexpr int FD_SLOTS = 64;                 // reviews a mask can remove (docs_masked_device.h)
constexpr int FD_MAX_T = 65536;
constexpr int FD_WAVES = 4;                  // waves (= rows in flight) per workgroup
constexpr int FD_MAX_BLOCKS = 8192;          // beyond, a workgroup's waves loop over rows
constexpr int FD_WINDOWS = 2 * FD_SLOTS + 2 + 5;   // a row's listed windows: two per review, the tail's, the end's
constexpr int FD_OUTSIDE = -1;               // a tap outside the document: a row of 0.0f
constexpr int FD_NONE = -2;                  // no window here (a one-word review's second): -inf
constexpr int FD_CHUNK = WAVE - 4;           // interior windows per 64 tokens read: a multiple of 4, two tokens of overlap
constexpr int FD_BATCH = 8;                  // listed windows whose rows are requested together

constexpr int FP_TILE = 64;                  // words x columns of a projection tile
constexpr int FP_K = 16;                     // its K chunk

// ---------------------------------------------------------------- projection
// ptab[v, j F + f] = sum_k table[v, k] conv_w[f, j, k], k ascending, one fmaf per term.
__global__ __launch_bounds__(256) void fold_project_kernel(const float *__restrict__ table, int64_t V,
                                                           const float *__restrict__ conv_w, float *__restrict__ ptab,
                                                           int E, int F, int PS) {
    __shared__ __attribute__((aligned(16))) float As[FP_K][FP_TILE + 4];
    __shared__ __attribute__((aligned(16))) float Bs[FP_K][FP_TILE + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t v0 = (int64_t)blockIdx.x * FP_TILE;
    const int c0 = blockIdx.y * FP_TILE, C = 3 * F;
    const int lr = tid >> 2, lk = (tid & 3) * 4;             // the loader's row of the tile and its four k
    const int64_t arow = v0 + lr;
    const int bcol = c0 + lr;
    const float *asrc = arow < V ? table + arow * E : nullptr;
    const float *bsrc = bcol < C ? conv_w + ((int64_t)(bcol % F) * 3 + bcol / F) * E : nullptr;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < E; k0 += FP_K) {
        const bool in = k0 + lk < E;                         // (E % 4 == 0: a float4 is inside or outside as a whole)
        const float4 av = asrc && in ? *reinterpret_cast<const float4 *>(asrc + k0 + lk) : make_float4(0, 0, 0, 0);
        const float4 bv = bsrc && in ? *reinterpret_cast<const float4 *>(bsrc + k0 + lk) : make_float4(0, 0, 0, 0);
        As[lk][lr] = av.x; As[lk + 1][lr] = av.y; As[lk + 2][lr] = av.z; As[lk + 3][lr] = av.w;
        Bs[lk][lr] = bv.x; Bs[lk + 1][lr] = bv.y; Bs[lk + 2][lr] = bv.z; Bs[lk + 3][lr] = bv.w;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FP_K; ++k) {
            const float4 a4 = *reinterpret_cast<const float4 *>(&As[k][ty * 4]);
            const float4 b4 = *reinterpret_cast<const float4 *>(&Bs[k][tx * 4]);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = v0 + ty * 4 + i;
        if (row >= V) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = c0 + tx * 4 + j;
            if (col < C) ptab[row * PS + col] = acc[i][j];
        }
    }
}

// ---------------------------------------------------------------- windows
// A lane's two filters: f0 = lane, f1 = lane + 64 (clamped for the address; `two` is wave-uniform).
struct FoldLane {
    const float *ptab;
    size_t PS;
    int F, f0, f1;
    bool two;
    float bias0, bias1;
};

__device__ __forceinline__ FoldLane fold_lane(const float *ptab, const float *conv_b, int F, int PS, int lane) {
    FoldLane c;
    c.ptab = ptab;
    c.PS = (size_t)PS;
    c.F = F;
    c.f0 = lane < F ? lane : F - 1;
    c.f1 = lane + WAVE < F ? lane + WAVE : F - 1;
    c.two = F > WAVE;
    c.bias0 = conv_b[c.f0];
    c.bias1 = conv_b[c.f1];
    return c;
}

// best = max(best, ((r0 + r1) + r2) + b) for the window over tokens (a, m, d); FD_OUTSIDE taps are 0.0f rows,
// a == FD_NONE is no window.  Branch-free: the loads of an unrolled run of windows go out together.
__device__ __forceinline__ void fold_window(const FoldLane &c, int a, int m, int d, float &best0, float &best1) {
    const float *ra = c.ptab + (size_t)(a < 0 ? 0 : a) * c.PS;
    const float *rm = c.ptab + (size_t)(m < 0 ? 0 : m) * c.PS + c.F;
    const float *rd = c.ptab + (size_t)(d < 0 ? 0 : d) * c.PS + 2 * c.F;
    {
        const float g0 = ra[c.f0], g1 = rm[c.f0], g2 = rd[c.f0];   // (row 0 for a tap outside: read, not used)
        const float x0 = a < 0 ? 0.0f : g0, x1 = m < 0 ? 0.0f : g1, x2 = d < 0 ? 0.0f : g2;
        const float y = ((x0 + x1) + x2) + c.bias0;
        best0 = fmaxf(best0, a == FD_NONE ? -INFINITY : y);
    }
    if (c.two) {
        const float g0 = ra[c.f1], g1 = rm[c.f1], g2 = rd[c.f1];   // (row 0 for a tap outside: read, not used)
        const float x0 = a < 0 ? 0.0f : g0, x1 = m < 0 ? 0.0f : g1, x2 = d < 0 ? 0.0f : g2;
        const float y = ((x0 + x1) + x2) + c.bias1;
        best1 = fmaxf(best1, a == FD_NONE ? -INFINITY : y);
    }
}

// The windows (r[q - 2], r[q - 1], r[q]), q in [2, v), of the v tokens at r.  r and v are wave-uniform; the tokens are
// read 64 at a time, one per lane, and handed out as scalars.
__device__ __forceinline__ void fold_interior(const FoldLane &c, const int32_t *r, int v, int lane, float &best0,
                                              float &best1) {
    for (int base = 0; base + 2 < v; base += FD_CHUNK) {
        const int t = base + lane < v ? r[base + lane] : 0;
        const int left = v - 2 - base;
        const int n = left < FD_CHUNK ? left : FD_CHUNK;
        for (int q0 = 0; q0 < n; q0 += 4) {                  // (a fixed inner count: readlane keeps a runtime one rolled)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = q0 + j;
                const int x = __builtin_amdgcn_readlane(t, q);
                fold_window(c, q < n ? x : FD_NONE, __builtin_amdgcn_readlane(t, q + 1),
                            __builtin_amdgcn_readlane(t, q + 2), best0, best1);
            }
        }
    }
}

__device__ __forceinline__ int64_t lane_value64(int64_t v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), lane);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ---------------------------------------------------------------- segments
struct SegmentsArgs {
    const float *ptab, *conv_b;
    const int32_t *tok;
    const int64_t *rev_off, *first, *ids;
    int64_t n;
    int S, F, PS;
    float *seg;
};

__global__ __launch_bounds__(FD_WAVES *WAVE) void fold_segments_kernel(const SegmentsArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const FoldLane c = fold_lane(a.ptab, a.conv_b, a.F, a.PS, lane);
    const int64_t total = a.n * a.S;
    for (int64_t w = (int64_t)blockIdx.x * FD_WAVES + wave; w < total; w += (int64_t)gridDim.x * FD_WAVES) {
        const int64_t i = w / a.S;
        const int s = (int)(w - i * a.S);
        const int64_t id = a.ids[i];
        const int64_t rb = id >= 0 ? a.first[id] : 0, re = id >= 0 ? a.first[id + 1] : 0;
        float best0 = -INFINITY, best1 = -INFINITY;
        if (s < re - rb) {
            const int64_t at = a.rev_off[rb + s], len = a.rev_off[rb + s + 1] - at;
            if (len >= 3) fold_interior(c, a.tok + at, (int)(len < INT32_MAX ? len : INT32_MAX), lane, best0, best1);
        }
        float *out = a.seg + w * a.F;
        if (lane < a.F) out[lane] = best0;
        if (lane + WAVE < a.F) out[lane + WAVE] = best1;
    }
}

// ---------------------------------------------------------------- compose
struct ComposeArgs {
    const float *ptab, *conv_b, *seg;
    const int32_t *tok;
    const int64_t *rev_off, *first, *row_owner, *ids, *drop;
    int64_t M;
    int S, T, F, PS;
    float *pooled;
};

__global__ __launch_bounds__(FD_WAVES *WAVE) void fold_compose_kernel(const ComposeArgs a) {
    __shared__ int4 swin[FD_WAVES][(FD_WINDOWS + FD_BATCH - 1) & ~(FD_BATCH - 1)];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    int4 *win = swin[wave];
    const FoldLane c = fold_lane(a.ptab, a.conv_b, a.F, a.PS, lane);
    const int T = a.T, S = a.S, F = a.F;
    for (int64_t m = (int64_t)blockIdx.x * FD_WAVES + wave; m < a.M; m += (int64_t)gridDim.x * FD_WAVES) {
        float *out = a.pooled + m * F;
        const int64_t o = a.row_owner[m];
        if (o < 0) {                                         // (wave-uniform) a row that is not computed
            if (lane < F) out[lane] = 0.0f;
            if (lane + WAVE < F) out[lane + WAVE] = 0.0f;
            continue;
        }
        const int64_t id = a.ids[o];
        const int64_t rb = id >= 0 ? a.first[id] : 0, re = id >= 0 ? a.first[id + 1] : 0;
        const int64_t count = re - rb;
        const uint64_t drop = a.drop ? (uint64_t)a.drop[m] : 0;
        // ---- lanes are review slots: kept lengths, their running sum, the first / last two tokens
        int64_t at = 0, full = 0;
        if (lane < count) {
            at = a.rev_off[rb + lane];
            full = a.rev_off[rb + lane + 1] - at;
        }
        const int64_t len = ((drop >> lane) & 1) ? 0 : full;
        int64_t sum = len;
#pragma unroll
        for (int d = 1; d < FD_SLOTS; d <<= 1) {
            const int64_t up = __shfl_up(sum, d, WAVE);
            if (lane >= d) sum += up;
        }
        const int64_t start = sum - len;
        const int64_t head = lane_value64(sum, FD_SLOTS - 1);
        const bool shows = len > 0 && start < T;
        const int v = shows ? (int)(len < T - start ? len : T - start) : 0;
        const uint64_t mask = __ballot(shows);
        const uint64_t cached = __ballot(shows && v == len && lane < S);
        const uint64_t walk = __ballot(shows && v >= 3) & ~cached;
        int r0 = FD_OUTSIDE, r1 = FD_OUTSIDE, l1 = FD_OUTSIDE, l2 = FD_OUTSIDE;
        if (shows) {
            const int32_t *r = a.tok + at;
            r0 = r[0];
            l1 = r[v - 1];
            if (v >= 2) {
                r1 = r[1];
                l2 = r[v - 2];
            }
        }
        // the two document tokens ahead of a review: the last of the showing review below it, and that review's
        // second to last or, where it has one word, the last of the showing review below that one
        const uint64_t below = mask & ((1ull << lane) - 1);
        const int i1 = below ? 63 - __clzll((long long)below) : -1;
        const uint64_t below2 = i1 >= 0 ? below & ~(1ull << i1) : 0;
        const int i2 = below2 ? 63 - __clzll((long long)below2) : -1;
        const int pl1 = __shfl(l1, i1 < 0 ? 0 : i1, WAVE), pl2 = __shfl(l2, i1 < 0 ? 0 : i1, WAVE);
        const int pv = __shfl(v, i1 < 0 ? 0 : i1, WAVE), ql1 = __shfl(l1, i2 < 0 ? 0 : i2, WAVE);
        const int p1 = i1 < 0 ? FD_OUTSIDE : pl1;
        const int p2 = i1 < 0 ? FD_OUTSIDE : pv >= 2 ? pl2 : i2 < 0 ? FD_OUTSIDE : ql1;
        wave_lds_fence();                                    // the reads of the row before are done
        if (shows) {
            const int at2 = 2 * __popcll(below);
            win[at2] = make_int4(p2, p1, r0, 0);
            win[at2 + 1] = v >= 2 ? make_int4(p1, r0, r1, 0) : make_int4(FD_NONE, FD_OUTSIDE, FD_OUTSIDE, 0);
        }
        // ---- wave-uniform: the state after the last showing review, the tail, the padding, the end
        int nwin = 2 * __popcll(mask);
        int e1 = FD_OUTSIDE, e2 = FD_OUTSIDE;
        if (mask) {
            const int j1 = 63 - __clzll((long long)mask);
            const uint64_t rest = mask & ~(1ull << j1);
            e1 = __builtin_amdgcn_readlane(l1, j1);
            if (__builtin_amdgcn_readlane(v, j1) >= 2) e2 = __builtin_amdgcn_readlane(l2, j1);
            else if (rest) e2 = __builtin_amdgcn_readlane(l1, 63 - __clzll((long long)rest));
        }
        int64_t pos = head < T ? head : T;
        const int64_t end = a.rev_off[re > rb ? re : rb];
        const int64_t tail_at = count > FD_SLOTS ? a.rev_off[rb + FD_SLOTS] : end;
        const int64_t tail_len = end - tail_at;
        const int tv = tail_len > 0 && head < T ? (int)(tail_len < T - head ? tail_len : T - head) : 0;
        if (tv > 0) {
            const int32_t *r = a.tok + tail_at;
            const int t0 = r[0], t1 = tv >= 2 ? r[1] : FD_OUTSIDE;
            if (lane == 0) {
                win[nwin] = make_int4(e2, e1, t0, 0);
                win[nwin + 1] = tv >= 2 ? make_int4(e1, t0, t1, 0) : make_int4(FD_NONE, FD_OUTSIDE, FD_OUTSIDE, 0);
            }
            nwin += 2;
            if (tv >= 2) {
                e2 = r[tv - 2];
                e1 = r[tv - 1];
            } else {
                e2 = e1;
                e1 = t0;
            }
            pos = head + tv;
        }
        const int npad = T - pos < 3 ? (int)(T - pos) : 3;
        for (int q = 0; q < npad + 2; ++q) {                 // up to three windows ending on word 0, two hanging over
            const int t = q < npad ? 0 : FD_OUTSIDE;
            if (lane == 0) win[nwin] = make_int4(e2, e1, t, 0);
            ++nwin;
            e2 = e1;
            e1 = t;
        }
        if (lane < FD_BATCH && nwin + lane < ((nwin + FD_BATCH - 1) & ~(FD_BATCH - 1)))
            win[nwin + lane] = make_int4(FD_NONE, FD_OUTSIDE, FD_OUTSIDE, 0);
        wave_lds_fence();
        // ---- lanes are filters
        float best0 = -INFINITY, best1 = -INFINITY;
        for (int w0 = 0; w0 < nwin; w0 += FD_BATCH) {
#pragma unroll
            for (int j = 0; j < FD_BATCH; ++j) {
                const int4 t = win[w0 + j];
                fold_window(c, __builtin_amdgcn_readfirstlane(t.x), __builtin_amdgcn_readfirstlane(t.y),
                            __builtin_amdgcn_readfirstlane(t.z), best0, best1);
            }
        }
        const int nseg = (int)(count < S ? count : S);
        const float *sg = a.seg + o * (int64_t)S * F;
#pragma unroll 8
        for (int s = 0; s < nseg; ++s) {
            const bool use = (cached >> s) & 1;
            const float x0 = sg[s * F + c.f0];
            best0 = fmaxf(best0, use ? x0 : -INFINITY);
            if (c.two) {
                const float x1 = sg[s * F + c.f1];
                best1 = fmaxf(best1, use ? x1 : -INFINITY);
            }
        }
        for (uint64_t left = walk; left; left &= left - 1) { // the review cut by T, reviews beyond seg's S slots
            const int s = __builtin_ctzll(left);
            fold_interior(c, a.tok + lane_value64(at, s), __builtin_amdgcn_readlane(v, s), lane, best0, best1);
        }
        if (tv >= 3) fold_interior(c, a.tok + tail_at, tv, lane, best0, best1);
        if (lane < F) out[lane] = best0 > 0.0f ? best0 : 0.0f;
        if (lane + WAVE < F) out[lane + WAVE] = best1 > 0.0f ? best1 : 0.0f;
    }
}

// ---------------------------------------------------------------- the search's bookkeeping
__device__ __forceinline__ bool fold_crossed(float score, float target, int direction) {
    return direction == 0 ? score < target : score > target; // strict; false for a NaN on either side
}

__global__ __launch_bounds__(256) void fold_search_begin_kernel(const float *score0, const float *target, int direction,
                                                                int B, int64_t n_p, int32_t *order, float *scores,
                                                                int32_t *steps, int32_t *crossed, int32_t *done) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_p) return;
    const float s = score0[p];
    for (int b = 0; b <= B; ++b) scores[p * (B + 1) + b] = s;
    for (int b = 0; b < B; ++b) order[p * B + b] = -1;
    const int hit = fold_crossed(s, target[p], direction) ? 1 : 0;
    steps[p] = 0;
    crossed[p] = hit;
    done[p] = hit;
}

struct SearchSide {
    const int64_t *rev_off, *first, *ids, *own, *mask, *cand;
    int S;
    int64_t *row_owner, *drop;
};

struct SearchRowsArgs {
    SearchSide u, i;
    const int32_t *done;
    int64_t n_p;
    int T;
};

// One side's columns [col0, col0 + S) of pair p's C candidate rows, and the fill of the other columns.
__device__ __forceinline__ void fold_search_side(const SearchSide &sd, bool live, int64_t p, int T, int C, int col0,
                                                 int lane) {
    if (sd.S == 0) return;
    const int64_t o = sd.own[p], id = sd.ids[o];
    const int64_t rb = id >= 0 ? sd.first[id] : 0, re = id >= 0 ? sd.first[id + 1] : 0;
    const uint64_t mask = (uint64_t)sd.mask[p], cand = sd.cand ? (uint64_t)sd.cand[p] : 0;
    const int64_t full = lane < re - rb ? sd.rev_off[rb + lane + 1] - sd.rev_off[rb + lane] : 0;
    const bool gone = (mask >> lane) & 1;
    const int64_t len = gone ? 0 : full;
    int64_t sum = len;
#pragma unroll
    for (int d = 1; d < FD_SLOTS; d <<= 1) {
        const int64_t up = __shfl_up(sum, d, WAVE);
        if (lane >= d) sum += up;
    }
    const uint64_t ok = __ballot(live && lane < sd.S && ((cand >> lane) & 1) && !gone && full > 0 && sum - len < T);
    for (int c = lane; c < C; c += WAVE) {
        const int s = c - col0;
        const bool is = s >= 0 && s < sd.S && ((ok >> s) & 1);
        sd.row_owner[p * C + c] = is ? o : -1;
        sd.drop[p * C + c] = (int64_t)(is ? mask | (1ull << s) : mask);
    }
}

__global__ __launch_bounds__(FD_WAVES *WAVE) void fold_search_rows_kernel(const SearchRowsArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int C = a.u.S + a.i.S;
    for (int64_t p = (int64_t)blockIdx.x * FD_WAVES + wave; p < a.n_p; p += (int64_t)gridDim.x * FD_WAVES) {
        const bool live = a.done[p] == 0;
        fold_search_side(a.u, live, p, a.T, C, 0, lane);
        fold_search_side(a.i, live, p, a.T, C, a.u.S, lane);
    }
}

struct SearchPickArgs {
    const float *cand_score, *target;
    const int64_t *row_owner_u, *row_owner_i;
    int S_u, S_i, direction, B, L;
    int64_t n_p;
    int64_t *mask_u, *mask_i;
    float *z_u, *z_i;
    int32_t *order, *steps, *crossed, *done;
    float *scores;
};

// Is candidate (sb, cb) better than (sa, ca)?  A column of -1 is no candidate.  A total order: every lane of the
// butterfly ends with the same winner.
__device__ __forceinline__ bool fold_better(float sa, int ca, float sb, int cb, int direction) {
    if (cb < 0) return false;
    if (ca < 0) return true;
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return na;
    if (na || sa == sb) return cb < ca;
    return direction == 0 ? sb < sa : sb > sa;
}

__global__ __launch_bounds__(FD_WAVES *WAVE) void fold_search_pick_kernel(const SearchPickArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const int C = a.S_u + a.S_i, B = a.B, L = a.L;
    for (int64_t p = (int64_t)blockIdx.x * FD_WAVES + wave; p < a.n_p; p += (int64_t)gridDim.x * FD_WAVES) {
        if (a.done[p]) continue;                             // (wave-uniform)
        float best = 0.0f;
        int col = -1;
        for (int c = lane; c < C; c += WAVE) {
            const bool is = c < a.S_u ? a.row_owner_u[p * C + c] >= 0 : a.row_owner_i[p * C + c] >= 0;
            const float s = a.cand_score[p * C + c];
            if (fold_better(best, col, s, is ? c : -1, a.direction)) {
                best = s;
                col = c;
            }
        }
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const float so = __shfl_xor(best, d, WAVE);
            const int co = __shfl_xor(col, d, WAVE);
            if (fold_better(best, col, so, co, a.direction)) {
                best = so;
                col = co;
            }
        }
        col = __builtin_amdgcn_readfirstlane(col);
        best = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, best)));
        if (col < 0) {                                       // no candidate left
            if (lane == 0) a.done[p] = 1;
            continue;
        }
        const int step = a.steps[p];
        const bool user = col < a.S_u;
        const int slot = user ? col : col - a.S_u;
        for (int b = step + 1 + lane; b <= B; b += WAVE) a.scores[p * (B + 1) + b] = best;
        float *z = user ? a.z_u : a.z_i;
        for (int l = lane; l < L; l += WAVE) z[p * L + l] = z[(a.n_p + p * C + col) * L + l];
        if (lane == 0) {
            int64_t *mask = user ? a.mask_u : a.mask_i;
            mask[p] = (int64_t)((uint64_t)mask[p] | (1ull << slot));
            a.order[p * B + step] = user ? slot : FD_SLOTS + slot;
            a.steps[p] = step + 1;
            const int hit = fold_crossed(best, a.target[p], a.direction) ? 1 : 0;
            a.crossed[p] = hit;
            a.done[p] = hit || step + 1 >= B ? 1 : 0;
        }
    }
}

static unsigned fold_blocks(int64_t waves) {
    const int64_t want = cdiv(waves, FD_WAVES);
    return (unsigned)(want < FD_MAX_BLOCKS ? want : FD_MAX_BLOCKS);
}

}  // namespace r4r

using namespace r4r;

extern "C" int r4r_fold_ptab_stride(int F) { return F >= 1 && F <= FD_MAXF ? (3 * F + 3) & ~3 : 0; }

extern "C" int r4r_fold_project(const float *table, int64_t V, const float *conv_w, float *ptab, int E, int F,
                                void *stream) {
    R4R_REQUIRE(F >= 1 && F <= FD_MAXF, "r4r_fold_project: F=%d filters outside 1..%d", F, FD_MAXF);
    R4R_REQUIRE(E > 0 && E % 4 == 0, "r4r_fold_project: word_embed_size %d must be a positive multiple of 4", E);
    R4R_REQUIRE(V >= 0 && V < (1ll << 31), "r4r_fold_project: V=%lld words outside 0..2^31-1", (long long)V);
    if (V == 0) return R4R_OK;
    R4R_REQUIRE(table && conv_w && ptab, "r4r_fold_project: null pointer");
    const dim3 grid((unsigned)cdiv(V, FP_TILE), (unsigned)cdiv(3 * F, FP_TILE));
    hipLaunchKernelGGL(fold_project_kernel, grid, dim3(256), 0, as_stream(stream), table, V, conv_w, ptab, E, F,
                       r4r_fold_ptab_stride(F));
    return check_launch("r4r_fold_project");
}

extern "C" int r4r_fold_segments(const float *ptab, const float *conv_b, const int32_t *tok, const int64_t *rev_off,
                                 const int64_t *first, const int64_t *ids, int64_t n, int S, int F, float *seg,
                                 void *stream) {
    R4R_REQUIRE(F >= 1 && F <= FD_MAXF, "r4r_fold_segments: F=%d filters outside 1..%d", F, FD_MAXF);
    R4R_REQUIRE(S >= 1 && S <= FD_SLOTS, "r4r_fold_segments: S=%d slots outside 1..%d", S, FD_SLOTS);
    R4R_REQUIRE(n >= 0 && n < (1ll << 31), "r4r_fold_segments: n=%lld owners outside 0..2^31-1", (long long)n);
    if (n == 0) return R4R_OK;
    R4R_REQUIRE(ptab && conv_b && tok && rev_off && first && ids && seg, "r4r_fold_segments: null pointer");
    SegmentsArgs a{ptab, conv_b, tok, rev_off, first, ids, n, S, F, r4r_fold_ptab_stride(F), seg};
    hipLaunchKernelGGL(fold_segments_kernel, dim3(fold_blocks(n * S)), dim3(FD_WAVES * WAVE), 0, as_stream(stream), a);
    return check_launch("r4r_fold_segments");
}

extern "C" int r4r_fold_compose(const float *ptab, const float *conv_b, const float *seg, int S, const int32_t *tok,
                                const int64_t *rev_off, const int64_t *first, const int64_t *row_owner,
                                const int64_t *ids, const int64_t *drop, int64_t M, int T, int F, float *pooled,
                                void *stream) {
    R4R_REQUIRE(F >= 1 && F <= FD_MAXF, "r4r_fold_compose: F=%d filters outside 1..%d", F, FD_MAXF);
    R4R_REQUIRE(S >= 1 && S <= FD_SLOTS, "r4r_fold_compose: S=%d slots outside 1..%d", S, FD_SLOTS);
    R4R_REQUIRE(T >= 1 && T <= FD_MAX_T, "r4r_fold_compose: T=%d words outside 1..%d", T, FD_MAX_T);
    R4R_REQUIRE(M >= 0 && M < (1ll << 31), "r4r_fold_compose: M=%lld rows outside 0..2^31-1", (long long)M);
    if (M == 0) return R4R_OK;
    R4R_REQUIRE(ptab && conv_b && seg && tok && rev_off && first && row_owner && ids && pooled,
                "r4r_fold_compose: null pointer");
    ComposeArgs a{ptab, conv_b, seg, tok, rev_off, first, row_owner, ids, drop, M, S, T, F, r4r_fold_ptab_stride(F), pooled};
    hipLaunchKernelGGL(fold_compose_kernel, dim3(fold_blocks(M)), dim3(FD_WAVES * WAVE), 0, as_stream(stream), a);
    return check_launch("r4r_fold_compose");
}

extern "C" int r4r_fold_search_begin(const float *score0, const float *target, int direction, int budget, int64_t n_p,
                                     int32_t *out_order, float *out_scores, int32_t *out_steps, int32_t *out_crossed,
                                     int32_t *done, void *stream) {
    R4R_REQUIRE(direction == 0 || direction == 1, "r4r_fold_search_begin: direction %d is neither 0 nor 1", direction);
    R4R_REQUIRE(budget >= 1 && budget <= FD_SLOTS, "r4r_fold_search_begin: budget=%d outside 1..%d", budget, FD_SLOTS);
    R4R_REQUIRE(n_p >= 0 && n_p * (budget + 1) < (1ll << 31), "r4r_fold_search_begin: n_p=%lld pairs at budget %d",
                (long long)n_p, budget);
    if (n_p == 0) return R4R_OK;
    R4R_REQUIRE(score0 && target && out_order && out_scores && out_steps && out_crossed && done,
                "r4r_fold_search_begin: null pointer");
    hipLaunchKernelGGL(fold_search_begin_kernel, dim3((unsigned)cdiv(n_p, 256)), dim3(256), 0, as_stream(stream), score0,
                       target, direction, budget, n_p, out_order, out_scores, out_steps, out_crossed, done);
    return check_launch("r4r_fold_search_begin");
}

static int check_search_sides(const char *who, int S_u, int S_i, int64_t n_p) {
    R4R_REQUIRE(S_u >= 0 && S_u <= FD_SLOTS && S_i >= 0 && S_i <= FD_SLOTS && S_u + S_i >= 1,
                "%s: S_u=%d, S_i=%d slots: each 0..%d, one at least 1", who, S_u, S_i, FD_SLOTS);
    R4R_REQUIRE(n_p >= 0 && n_p * (S_u + S_i + 1) < (1ll << 31), "%s: n_p=%lld pairs of %d candidates", who,
                (long long)n_p, S_u + S_i);
    return R4R_OK;
}

extern "C" int r4r_fold_search_rows(const int64_t *rev_off_u, const int64_t *first_u, const int64_t *ids_u,
                                    const int64_t *own_u, const int64_t *mask_u, const int64_t *cand_u, int S_u,
                                    const int64_t *rev_off_i, const int64_t *first_i, const int64_t *ids_i,
                                    const int64_t *own_i, const int64_t *mask_i, const int64_t *cand_i, int S_i,
                                    const int32_t *done, int64_t n_p, int T, int64_t *row_owner_u, int64_t *drop_u,
                                    int64_t *row_owner_i, int64_t *drop_i, void *stream) {
    if (int rc = check_search_sides("r4r_fold_search_rows", S_u, S_i, n_p)) return rc;
    R4R_REQUIRE(T >= 1 && T <= FD_MAX_T, "r4r_fold_search_rows: T=%d words outside 1..%d", T, FD_MAX_T);
    if (n_p == 0) return R4R_OK;
    R4R_REQUIRE(done, "r4r_fold_search_rows: null done");
    R4R_REQUIRE(S_u == 0 || (rev_off_u && first_u && ids_u && own_u && mask_u && row_owner_u && drop_u),
                "r4r_fold_search_rows: null pointer on the user side");
    R4R_REQUIRE(S_i == 0 || (rev_off_i && first_i && ids_i && own_i && mask_i && row_owner_i && drop_i),
                "r4r_fold_search_rows: null pointer on the item side");
    SearchRowsArgs a{{rev_off_u, first_u, ids_u, own_u, mask_u, cand_u, S_u, row_owner_u, drop_u},
                     {rev_off_i, first_i, ids_i, own_i, mask_i, cand_i, S_i, row_owner_i, drop_i}, done, n_p, T};
    hipLaunchKernelGGL(fold_search_rows_kernel, dim3(fold_blocks(n_p)), dim3(FD_WAVES * WAVE), 0, as_stream(stream), a);
    return check_launch("r4r_fold_search_rows");
}

extern "C" int r4r_fold_search_pick(const float *cand_score, const int64_t *row_owner_u, const int64_t *row_owner_i,
                                    int S_u, int S_i, const float *target, int direction, int budget, int64_t n_p,
                                    int64_t *mask_u, int64_t *mask_i, float *z_u, float *z_i, int L, int32_t *out_order,
                                    float *out_scores, int32_t *out_steps, int32_t *out_crossed, int32_t *done,
                                    void *stream) {
    if (int rc = check_search_sides("r4r_fold_search_pick", S_u, S_i, n_p)) return rc;
    R4R_REQUIRE(direction == 0 || direction == 1, "r4r_fold_search_pick: direction %d is neither 0 nor 1", direction);
    R4R_REQUIRE(budget >= 1 && budget <= FD_SLOTS, "r4r_fold_search_pick: budget=%d outside 1..%d", budget, FD_SLOTS);
    R4R_REQUIRE(L >= 1, "r4r_fold_search_pick: L=%d, at least 1", L);
    if (n_p == 0) return R4R_OK;
    R4R_REQUIRE(cand_score && target && out_order && out_scores && out_steps && out_crossed && done,
                "r4r_fold_search_pick: null pointer");
    R4R_REQUIRE(S_u == 0 || (row_owner_u && mask_u && z_u), "r4r_fold_search_pick: null pointer on the user side");
    R4R_REQUIRE(S_i == 0 || (row_owner_i && mask_i && z_i), "r4r_fold_search_pick: null pointer on the item side");
    SearchPickArgs a{cand_score, target, row_owner_u, row_owner_i, S_u, S_i, direction, budget, L, n_p, mask_u, mask_i,
                     z_u, z_i, out_order, out_steps, out_crossed, done, out_scores};
    hipLaunchKernelGGL(fold_search_pick_kernel, dim3(fold_blocks(n_p)), dim3(FD_WAVES * WAVE), 0, as_stream(stream), a);
    return check_launch("r4r_fold_search_pick");
}

// Token state of the project-then-gather conv (project.hip): mark the tokens a batch uses,
// compact them into dense rows.  Per-workgroup bodies, shared by the stand-alone kernels
// (project.hip) and by the fused DeepCoNN step (engine.hip), which runs them for the NEXT
// batch inside the backward / reduce launches of the current one.
#pragma once
#include "textcnn.h"

namespace r4r {

struct TokenTower {
    const int64_t *idx;          // [N, T]
    int *flags, *slot, *list, *count;   // as in ProjTower
};
struct TokenArgs {
    TokenTower t[MAX_TOWERS];
    int64_t N, V;
    int T, ntower;
};

// ---- mark: block `blk` of `nblk` blocks of `nthreads` threads, all towers
__device__ __forceinline__ void token_mark_block(const TokenArgs &a, int blk, int nblk, int nthreads) {
    const int64_t total = a.N * a.T;
    for (int t = 0; t < a.ntower; ++t) {
        const int64_t *__restrict__ idx = a.t[t].idx;
        int *__restrict__ flags = a.t[t].flags;
        for (int64_t i = (int64_t)blk * nthreads + threadIdx.x; i < total; i += (int64_t)nblk * nthreads)
            flags[idx[i]] = 1;
    }
}

// ---- compact: slot[v] = dense row id of token v (or -1), list[row] = v, count.
// A workgroup of NW waves owns 256 NW G consecutive tokens (G int4 of flags per thread, all
// loaded up front), scans its flags in LDS and reserves a contiguous row range with ONE
// atomicAdd on the tower's counter (G > 1 keeps the number of atomics on that one address in
// the low hundreds at V = 1M).  The order in which workgroups reserve ranges varies from run to
// run, but any token <-> row bijection gives bit-identical results downstream (a projected row
// depends only on its own token), so no global scan or sort is needed.  Flags are cleared as
// they are consumed; `count` is reset by the gather kernel: both are all-zero between uses.
template <int NW, int G = 1>
__device__ __forceinline__ void token_compact_block(const TokenTower &tw, int64_t V, int blk) {
    __shared__ int wsum[G * NW];
    __shared__ int base_row;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t g0 = (int64_t)blk * (64 * NW * G) + tid;  // int4 group g0 + 64 NW g: tokens 4 gi .. 4 gi + 3
    const int64_t ngroups = (V + 3) / 4;                    // flags / slot buffers are padded to 4
    int4 f[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t gi = g0 + (int64_t)g * (64 * NW);
        f[g] = make_int4(0, 0, 0, 0);
        if (gi < ngroups) f[g] = reinterpret_cast<int4 *>(tw.flags)[gi];
    }
    // exclusive prefix of the counts inside the workgroup: wave scans + (G NW)-entry LDS scan
    int cnt[G], incl[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        cnt[g] = f[g].x + f[g].y + f[g].z + f[g].w;
        incl[g] = cnt[g];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl[g], off);
            if (lane >= off) incl[g] += up;
        }
        if (lane == 63) wsum[g * NW + wave] = incl[g];
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int w = 0; w < G * NW; ++w) { const int c = wsum[w]; wsum[w] = run; run += c; }
        base_row = run ? atomicAdd(tw.count, run) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int64_t gi = g0 + (int64_t)g * (64 * NW);
        if (gi >= ngroups) continue;
        int at = base_row + wsum[g * NW + wave] + incl[g] - cnt[g];
        const int fl[4] = {f[g].x, f[g].y, f[g].z, f[g].w};
        int sl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sl[k] = -1;
            if (fl[k]) { sl[k] = at; tw.list[at] = (int)(gi * 4 + k); ++at; }
        }
        *reinterpret_cast<int4 *>(tw.slot + gi * 4) = make_int4(sl[0], sl[1], sl[2], sl[3]);
        if (cnt[g]) reinterpret_cast<int4 *>(tw.flags)[gi] = make_int4(0, 0, 0, 0);
    }
}
// Groups per thread inside the fused reduce launches: 8 for a large vocabulary (V = 1M: 123 instead of 977
// atomics per tower on one counter, reduce launch 30 -> 13 us), 1 otherwise (at V = 50k seven workgroups of
// eight loads each were 0.9 us SLOWER than 49 of one).
constexpr int COMPACT_BIG_G = 8;
constexpr int64_t COMPACT_BIG_V = 262144;
static inline int compact_groups(int64_t V) { return V > COMPACT_BIG_V ? COMPACT_BIG_G : 1; }
template <int NW>
__device__ __forceinline__ void token_compact_auto(const TokenTower &tw, int64_t V, int blk) {
    if (V > COMPACT_BIG_V) token_compact_block<NW, COMPACT_BIG_G>(tw, V, blk);   // uniform
    else token_compact_block<NW, 1>(tw, V, blk);
}

// ---- segment plan of the gather-add-max (project.hip): which 128-position segments of the NEXT batch are LIVE.
// Segment u of a tower (document-major, u = doc * tiles + seg, as the gather numbers them) is UNIFORM when every token
// of its window 128 seg - 2 .. p_hi - 1 names the same row -- the zero-padded tail of a document -- with tokens outside
// the document a row of their own (the rule the gather's `same` applies per slice: a document's first and last segment
// are live); such a segment is decided in one round by each of its workers, a live one is walked.  The gather pairs one
// live with one uniform segment per workgroup from `perm`, the stable partition "live first".  The flags steer the
// schedule only: `perm` is a permutation of 0 .. units - 1 whatever `live` holds.
constexpr int PLAN_SEG = 128;               // = project.hip's SEG
constexpr int PLAN_MAX_UNITS = 4096;        // one workgroup scans a tower's flags; `live` and `perm` are carved at this size
struct PlanArgs {
    const int64_t *idx[2];       // [N, T] of the next batch, per tower
    int *live[2];                // [PLAN_MAX_UNITS] all-zero between uses (set by the flag role, cleared by the scan)
    int *perm[2];                // [PLAN_MAX_UNITS]
    int *plan_ready[2];          // [1]
    int T, tiles, units;         // units = N * tiles per tower; 0: no plan is made
};

// flags: one wave per segment, wave g of 2 * units (tower-major).  No atomics: one lane stores the segment's flag.
__device__ __forceinline__ void segment_flags_wave(const PlanArgs &p, int g) {
    const int lane = threadIdx.x & 63;
    const int t = g >= p.units, u = g - t * p.units;
    if (u >= p.units) return;
    const int doc = u / p.tiles, seg = u - doc * p.tiles, T = p.T;
    const int t_lo = PLAN_SEG * seg - 2, t_hi = min(T + 2, PLAN_SEG * (seg + 1));   // tokens t_lo .. t_hi - 1: at most 130
    const int64_t *__restrict__ row = (t ? p.idx[1] : p.idx[0]) + (int64_t)doc * T;
    // lane l takes tokens t_lo + l, + 64 and (l < 2) + 128, all requested together
    long long v[3];
    bool valid[3], in[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int tk = t_lo + 64 * k + lane;
        valid[k] = tk < t_hi && (k < 2 || lane < 2);
        in[k] = valid[k] && tk >= 0 && tk < T;
        v[k] = row[in[k] ? tk : 0];
    }
    bool differs = false;
    long long first = in[0] ? v[0] : -1;
    first = __shfl(first, 0);                                // token t_lo: the window's first
#pragma unroll
    for (int k = 0; k < 3; ++k) differs |= valid[k] && (in[k] ? v[k] : -1) != first;
    if (__ballot(differs) != 0ull && lane == 0) (t ? p.live[1] : p.live[0])[u] = 1;
}

// plan: ONE workgroup of NT threads per tower.  Thread i owns units K i .. K i + K - 1 (K = PLAN_MAX_UNITS / NT, loaded
// as int4s up front); an exclusive prefix of the live counts over the workgroup places the live units, in order, at
// perm[0 .. nlive) and the uniform ones, in order, behind them.  `live` is cleared as it is consumed; plan_ready is
// written last, 1 only where the plan is worth its extra round trip in the gather: an eighth of the units uniform.
template <int NT>
__device__ __forceinline__ void segment_plan_block(const PlanArgs &p, int t) {
    constexpr int K = PLAN_MAX_UNITS / NT, NW = NT / 64;
    static_assert(K % 4 == 0 && NT % 64 == 0, "int4 loads of whole waves");
    __shared__ int wtot[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, units = p.units;
    int *__restrict__ live = t ? p.live[1] : p.live[0];
    int *__restrict__ perm = t ? p.perm[1] : p.perm[0];
    int f[K];
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
        const int4 x = reinterpret_cast<const int4 *>(live)[tid * (K / 4) + q];
        f[4 * q] = x.x; f[4 * q + 1] = x.y; f[4 * q + 2] = x.z; f[4 * q + 3] = x.w;
    }
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        f[k] = (f[k] != 0 && tid * K + k < units) ? 1 : 0;
        cnt += f[k];
    }
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int before = incl - cnt, nlive = 0;                      // live units in front of this thread's first; of the tower
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int c = wtot[w];
        if (w < wave) before += c;
        nlive += c;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int u = tid * K + k;
        if (u < units) perm[f[k] ? before : nlive + (u - before)] = u;
        before += f[k];
    }
    if (cnt) {
#pragma unroll
        for (int q = 0; q < K / 4; ++q) reinterpret_cast<int4 *>(live)[tid * (K / 4) + q] = make_int4(0, 0, 0, 0);
    }
    __syncthreads();
    if (tid == 0) (t ? p.plan_ready[1] : p.plan_ready[0])[0] = ((units - nlive) * 8 >= units) ? 1 : 0;
}

static inline TokenArgs make_token_args(int64_t V, const ProjTower *tw, int ntower, int64_t N, int T) {
    TokenArgs a;
    for (int k = 0; k < MAX_TOWERS; ++k) {
        const ProjTower &s = tw[k < ntower ? k : 0];
        a.t[k].idx = s.idx; a.t[k].flags = s.flags; a.t[k].slot = s.slot; a.t[k].list = s.list; a.t[k].count = s.count;
    }
    a.N = N; a.V = V; a.T = T; a.ntower = ntower;
    return a;
}

}  // namespace r4r

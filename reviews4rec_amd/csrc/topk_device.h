// What the catalogue scans share (topk.hip: r4r_topk_dot / r4r_rank_dot, topk_relu.hip: r4r_topk_relu / r4r_rank_relu):
// the result order, the sorted per-query list of one wave, and the merge of the chunks' partial lists.
#pragma once
#include <math.h>

#include "common.h"

namespace r4r {

constexpr int TOPK_MAX_K = 128;
constexpr int64_t TOPK_MAX_CHUNK = (int64_t)1 << 30;
constexpr int TOPK_TARGET_WAVES = 4096;      // 256 CUs x 16 waves
constexpr int64_t TOPK_MIN_CHUNK = 512;      // below this the partial lists cost more than the scan saves
constexpr int MERGE_THREADS = 256;

// a is ahead of b in the result order
template <class IdT>
__device__ __forceinline__ bool ahead(float sa, IdT ia, float sb, IdT ib) { return sa > sb || (sa == sb && ia < ib); }

template <class IdT> struct fill_id;
template <> struct fill_id<int> { static constexpr int value = 0x7fffffff; };
template <> struct fill_id<int64_t> { static constexpr int64_t value = 0x7fffffffffffffffLL; };

__device__ __forceinline__ float lane_value(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// All 64 lanes of one wave insert (s, i) into the sorted list sc / id of K <= 128 slots (two per lane); unused slots hold
// (-inf, fill_id): never ahead of a real entry, so the list needs no count and its K-th score -- what a newcomer has to
// beat, -inf while there is room -- is sc[K - 1].  Returns that score as it is after the call.  One LDS round trip:
// every lane reads its slots, a ballot gives the position, the tail moves up by one out of registers.
template <class IdT>
__device__ __forceinline__ float list_insert(float *sc, IdT *id, int K, float s, IdT i, int lane) {
    const int p0 = lane, p1 = lane + 64;
    float e0 = -INFINITY, e1 = -INFINITY;
    IdT i0 = fill_id<IdT>::value, i1 = fill_id<IdT>::value;
    if (p0 < K) { e0 = sc[p0]; i0 = id[p0]; }
    if (p1 < K) { e1 = sc[p1]; i1 = id[p1]; }
    const bool b0 = p0 < K && ahead<IdT>(e0, i0, s, i);
    const bool b1 = p1 < K && ahead<IdT>(e1, i1, s, i);
    const int pos = __popcll(__ballot(b0)) + __popcll(__ballot(b1));
    if (pos >= K) return lane_value(K > 64 ? e1 : e0, (K - 1) & 63);          // (wave-uniform) not among the K best
    wave_lds_fence();
    if (p0 < K && !b0 && p0 + 1 < K) { sc[p0 + 1] = e0; id[p0 + 1] = i0; }
    if (p1 < K && !b1 && p1 + 1 < K) { sc[p1 + 1] = e1; id[p1 + 1] = i1; }
    if (lane == 0) { sc[pos] = s; id[pos] = i; }
    wave_lds_fence();
    if (pos == K - 1) return s;
    return lane_value(K - 2 >= 64 ? e1 : e0, (K - 2) & 63);                     // the old entry K - 2 is the new K - 1
}

// topk.hip: enqueue topk_merge_kernel over partial lists ps / pi [n_q, parts, K] -> out_ids / out_scores [n_q, K]
int topk_launch_merge(const float *ps, const int64_t *pi, int64_t n_q, int64_t parts, int K, int64_t *out_ids,
                      float *out_scores, hipStream_t st);

}  // namespace r4r

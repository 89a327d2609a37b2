// One row of a what-if document block (include/r4r.h, "What-if documents"): docs_device.h's write_doc with the one
// `skip` generalised to a SET of removed reviews -- bit s of `drop` takes the owner's s-th review away, s < 64 -- and a
// set of occluded positions that hold word 0, the padding the model already knows.  Every lane of the workgroup calls
// write_doc_masked with the same arguments, as docs_device.h's writers are called.
//
// The first wave reads the up to 64 review lengths, zeroes the dropped ones and leaves their inclusive prefix sum in LDS
// (`sum`), next to `delta[s]` = where review s starts in the pool minus where it starts in the document; reviews from the
// 65th on are never dropped and form one contiguous tail that starts at `tail` (entry 64 of the sums' table, in the
// pool's token coordinates) and ends at `end`.  A position p then finds its review by a six-step search over the 64
// sums, or lies in the tail.  The occluded positions are staged as one bit each in `flag`.  Each thread writes every
// element of its positions exactly once -- the token, 0 past the end, 0 where flagged -- so no two stores of a launch
// share an address and no order between stores is relied on.  Nothing outside [rev_off[rb], rev_off[re]) of `tok` is
// read, whatever `drop` and `occ` hold.
#pragma once
#include "common.h"

namespace r4r {

constexpr int VARIANT_SLOTS = 64;            // reviews a mask can remove: one bit of an int64 each
constexpr int VARIANT_MAX_T = 65536;         // the longest document: one flag bit per position, 8 KB of LDS

struct MaskedDocLds {
    int64_t sum[VARIANT_SLOTS];              // inclusive sums of the kept lengths of reviews 0 .. 63
    int64_t delta[VARIANT_SLOTS];            // rev_off[rb + s] - (sum[s] - kept length of s)
    int64_t tail, end;                       // the tail's first token and the owner's last + 1, in the pool
    uint32_t flag[VARIANT_MAX_T / 32];       // bit p % 32 of word p / 32: position p is occluded
};

// occ [n_occ]: positions to occlude (any value; outside [0, T) ignored, repeats harmless); n_occ == 0: none, occ unread
__device__ __forceinline__ void write_doc_masked(const int32_t *tok, const int64_t *rev_off, int64_t rb, int64_t re,
                                                 uint64_t drop, const int32_t *occ, int64_t n_occ, int T, int64_t *dst,
                                                 MaskedDocLds &s) {
    const int64_t count = re - rb;
    if (threadIdx.x < VARIANT_SLOTS) {
        const int lane = threadIdx.x;
        int64_t at = 0, len = 0;
        if (lane < count) {
            at = rev_off[rb + lane];
            if (!((drop >> lane) & 1)) len = rev_off[rb + lane + 1] - at;
        }
        int64_t v = len;
#pragma unroll
        for (int d = 1; d < VARIANT_SLOTS; d <<= 1) {
            const int64_t o = __shfl_up(v, d, WAVE);
            if (lane >= d) v += o;
        }
        s.sum[lane] = v;
        s.delta[lane] = at - (v - len);
        if (lane == 0) {
            s.end = rev_off[re > rb ? re : rb];
            s.tail = count > VARIANT_SLOTS ? rev_off[rb + VARIANT_SLOTS] : s.end;
        }
    }
    const int words = (T + 31) >> 5;
    if (n_occ > 0) {                         // (uniform over the workgroup)
        for (int w = threadIdx.x; w < words; w += blockDim.x) s.flag[w] = 0;
        __syncthreads();
        for (int64_t j = threadIdx.x; j < n_occ; j += blockDim.x) {
            const int p = occ[j];
            if (p >= 0 && p < T) atomicOr(&s.flag[p >> 5], 1u << (p & 31));
        }
    }
    __syncthreads();
    const int64_t head = s.sum[VARIANT_SLOTS - 1], tail = s.tail, end = s.end;
    for (int p = threadIdx.x; p < T; p += blockDim.x) {
        int64_t src;
        if (p < head) {
            int lo = 0;                      // the number of sums <= p: the review that holds position p
#pragma unroll
            for (int step = VARIANT_SLOTS / 2; step >= 1; step >>= 1)
                if (s.sum[lo + step - 1] <= p) lo += step;
            src = p + s.delta[lo];
        } else {
            src = tail + (p - head);
            if (src >= end) src = -1;
        }
        int64_t v = src >= 0 ? (int64_t)tok[src] : 0;
        if (n_occ > 0 && ((s.flag[p >> 5] >> (p & 31)) & 1)) v = 0;
        dst[p] = v;
    }
}

}  // namespace r4r

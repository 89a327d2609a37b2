// One row of a document block from a token pool (reviews4rec_amd/data.py holds the layout): what r4r_batch_build
// (batcher.hip) writes per (rating, slot) and r4r_tower_build (tower_span.hip) per owner.  Every lane of the workgroup
// calls these with the same arguments; lanes walk the row's output positions, so the stores are coalesced 8-byte writes
// and the token reads contiguous runs.  Nothing outside [rev_off[rb], rev_off[re]) of `tok` and [rb, re) of `nb` is read.
#pragma once
#include "common.h"

namespace r4r {

constexpr int NEIGHBOURS = 10;

// tokens of reviews [rb, re) of a pool minus review rb + skip, as a [T] document
__device__ __forceinline__ void write_doc(const int32_t *tok, const int64_t *rev_off, int64_t rb, int64_t re,
                                          int64_t skip, int T, int64_t *dst) {
    if (skip >= re - rb) skip = -1;      // an index past this owner's list removes nothing (data.py:223-235: `i != indices[k]` holds for every i)
    const int64_t start = rev_off[rb], end = rev_off[re > rb ? re : rb];
    int64_t hb = end, hl = 0;
    if (skip >= 0) {
        hb = rev_off[rb + skip];
        hl = rev_off[rb + skip + 1] - hb;
    }
    for (int p = threadIdx.x; p < T; p += blockDim.x) {
        int64_t src = start + p;
        if (src >= hb) src += hl;
        dst[p] = src < end ? (int64_t)tok[src] : 0;
    }
}

// the same reviews in NARRE's [R, W] layout: slot r = the r-th remaining review, cut / padded to W
__device__ __forceinline__ void write_reviews(const int32_t *tok, const int64_t *rev_off, int64_t rb, int64_t re,
                                              int64_t skip, int R, int W, int64_t *dst) {
    if (skip >= re - rb) skip = -1;
    for (int p = threadIdx.x; p < R * W; p += blockDim.x) {
        const int r = p / W, w = p - r * W;
        const int64_t rev = rb + r + ((skip >= 0 && r >= skip) ? 1 : 0);
        int64_t v = 0;
        if (rev < re) {
            const int64_t rs = rev_off[rev];
            if (w < rev_off[rev + 1] - rs) v = tok[rs + w];
        }
        dst[p] = v;
    }
}

__device__ __forceinline__ void write_neighbours(const int64_t *nb, int64_t rb, int64_t re, int64_t skip,
                                                 int64_t pad, int64_t *dst) {
    if (skip >= re - rb) skip = -1;
    if (threadIdx.x < NEIGHBOURS) {
        const int r = threadIdx.x;
        const int64_t at = rb + r + ((skip >= 0 && r >= skip) ? 1 : 0);
        dst[r] = at < re ? nb[at] : pad;
    }
}

}  // namespace r4r

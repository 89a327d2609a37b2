// Catalogue top-K and ranks over a product-FM head: r4r_topk_pfm / r4r_pair_pfm / r4r_rank_pfm (include/r4r.h,
// "Catalogue recommendation: product-FM heads").
//
//   x_m = fmaxf(q[u][m] + c[i][m], 0)   m < H          x_m = q[u][m] * c[i][m]   H <= m < D = H + G
//   y_j = fmaf(W[j][m], x_m, y_j)   m ascending, then y_j = y_j + b[j]                              j < M
//   t_k = fmaf(s[j] * y_j, y_j, t_k)               over the j with ((j >> 2) & 3) == k, ascending
//   v_k = fmaf(fmaf(g[m], x_m, e[m]), x_m, v_k)    over the m with (m & 3) == k, ascending
//   score(u, i) = (((((t_0 + v_0) + (t_1 + v_1)) + ((t_2 + v_2) + (t_3 + v_3))) + c_bias[i]) + q_bias[u])
//
// topk_rfm.hip's scan with three changes.  The columns behind H are PRODUCTS q * c; every column also feeds a per-column
// quadratic x (g x + e), summed by the lane that formed x; and the head lives in LDS, shared by the four waves of a
// workgroup, because at the limits (128 x 128) its 256 A fragments per lane do not fit a register file.
// Launch 1, pfm_scan_kernel: a workgroup of PFM_WAVES waves = PFM_WAVES consecutive tiles of QT queries x ONE chunk of
// candidates (with one or two tiles in the call: that many tiles x four or two neighbouring chunks, so that every SIMD
// of the CU has its wave).  All threads write the head's image, one barrier, then every wave runs on its own (a wave whose tile lies
// past the last one leaves): no barrier in the candidate loop.
//   image  W in FRAGMENT order: float 4 (64 (tq MT + mt) + l) + tt holds W[16 mt + (l & 15)][4 (4 tq + tt) + (l >> 4)],
//          zero beyond M and D.  Lane l's A values of the four MFMA steps 4 tq .. 4 tq + 3 of row tile mt are ONE aligned
//          ds_read_b128, and the 64 lanes read 64 consecutive 16-byte words: every group of lanes that the LDS serves
//          together covers all banks once.  Behind it b and s by row (lane group kq reads rows 16 mt + 4 kq .. + 3 as one
//          b128, a broadcast within the group) and g and e in the same step-major order as W.
//   A  read from the image inside the step loop, one b128 per (tq, mt), used by 4 steps x QT queries = 16 MFMAs; the
//      reads of group tq + 1 are issued before the MFMAs of group tq (PfmTile::scores)
//   B  lane l loads c[slab + (l & 15)][4 t + (l >> 4)] and forms x against its query's value (registers; LDS from KT = 16
//      on): per group of four steps v_add + v_max where all 16 columns lie below H, one v_mul where all lie at or behind
//      it (both wave-uniform), both and a per-lane select in the one group that straddles H; two fmaf per step and query
//      carry the lane's share v_kq of the column sum
//   C  lane l holds y of rows 16 mt + 4 (l >> 4) + r for candidate l & 15: the epilogue adds b, runs the t chain of ITS
//      lane group, adds v of the same group, two cross-lane adds (xor 16, xor 32: both orders of either add give the same
//      bits) finish the sum, then the two biases.  A row at or behind M is taken as y = 0 whatever its accumulator holds.
// The lists, the merge, the rank's three launches and the scalar kernels are topk_device.h's, over this file's PfmHead.
#include <math.h>

#include "common.h"
#include "slate_device.h"
#include "topk_device.h"

namespace r4r {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PFM_MAX_H = 64;
constexpr int PFM_MAX_G = 64;
constexpr int PFM_MAX_M = 128;
constexpr int PFM_QT = 4;          // queries (pairs) per wave, in every instantiation; the chunk rule counts with it too
constexpr int PFM_WAVES = 4;       // waves per workgroup: the tiles that share one image of the head
constexpr size_t PFM_STATIC_LDS = 64 * 1024;      // what a launch may ask for without the function attribute

// the scalar chain of one pair: q, c point at the pair's rows
__device__ __forceinline__ float pfm_pair_score(const float *q, const float *c, const float *W, const float *b, const float *s,
                                                const float *g, const float *e, int H, int D, int M, float cb, float qb) {
    float t[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < M; j0 += 16) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 4 * k + r;
                if (j >= M) break;
                const float *Wj = W + (size_t)j * D;
                float y = 0.f;
                for (int m = 0; m < H; ++m) y = __builtin_fmaf(Wj[m], __builtin_fmaxf(q[m] + c[m], 0.f), y);
                for (int m = H; m < D; ++m) y = __builtin_fmaf(Wj[m], q[m] * c[m], y);
                y = y + (b != nullptr ? b[j] : 0.f);
                const float sy = s[j] * y;
                t[k] = __builtin_fmaf(sy, y, t[k]);
            }
        }
    }
    for (int m0 = 0; m0 < D; m0 += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int m = m0 + k;
            if (m < D) {
                const float x = m < H ? __builtin_fmaxf(q[m] + c[m], 0.f) : q[m] * c[m];
                const float gm = g != nullptr ? g[m] : 0.f, em = e != nullptr ? e[m] : 0.f;
                v[k] = __builtin_fmaf(__builtin_fmaf(gm, x, em), x, v[k]);
            }
        }
    }
    return ((((t[0] + v[0]) + (t[1] + v[1])) + ((t[2] + v[2]) + (t[3] + v[3]))) + cb) + qb;
}

// The head of this form (topk_device.h); the two streams read its fields
struct PfmHead {
    const float *q, *q_bias, *c, *c_bias, *W, *b, *s, *g, *e;
    int64_t n_c, c_stride;
    int H, G, M, D;           // D = H + G

    __device__ __forceinline__ float q_bias_of(int64_t u) const { return q_bias ? q_bias[u] : 0.f; }
    __device__ __forceinline__ float score(int64_t u, int64_t i, float qb) const {
        return pfm_pair_score(q + u * D, c + i * c_stride, W, b, s, g, e, H, D, M, c_bias ? c_bias[i] : 0.f, qb);
    }
    __device__ __forceinline__ float score(int64_t u, int64_t i) const { return score(u, i, q_bias_of(u)); }

    static constexpr const char *width_name = "H + G";
    int width() const { return D; }
    int ranges(const char *fn) const {
        R4R_REQUIRE(H >= 0 && H <= PFM_MAX_H, "%s: H = %d outside 0 .. %d", fn, H, PFM_MAX_H);
        R4R_REQUIRE(G >= 0 && G <= PFM_MAX_G, "%s: G = %d outside 0 .. %d", fn, G, PFM_MAX_G);
        R4R_REQUIRE(M >= 0 && M <= PFM_MAX_M, "%s: M = %d outside 0 .. %d", fn, M, PFM_MAX_M);
        return R4R_OK;
    }
    int weights(const char *fn) const {
        R4R_REQUIRE(M == 0 || (W != nullptr && s != nullptr), "%s: null W or s with M > 0", fn);
        return R4R_OK;
    }
};

// The head's image in LDS and what a wave does with it.  KT: MFMA steps over the input width (D <= 4 KT), MT: 16-row
// tiles of y (M <= 16 MT); the image is padded to whole groups of four steps (KG of them).
template <int KT, int MT>
struct PfmTile {
    static constexpr int QT = PFM_QT;
    static constexpr int KG = (KT + 3) / 4;
    static constexpr int W_FLOATS = KG * MT * 256, ROW_FLOATS = MT * 16, COL_FLOATS = KG * 16;
    static constexpr int HEAD_FLOATS = W_FLOATS + 2 * ROW_FLOATS + 2 * COL_FLOATS;
    // QLDS: the wave's query rows live in LDS too (step-major, as g and e), not in QT x KT registers
    static constexpr bool QLDS = KT >= 16;
    static constexpr int QR = QLDS ? 1 : KT;                   // query registers per query
    static constexpr int Q_FLOATS = QLDS ? QT * COL_FLOATS : 0;                // per wave

    const f32x4 *wi, *bi, *si, *gi, *ei, *qi;  // the image (and the wave's query rows), as 16-byte words
    int lane, row, kq, H, D, mleft;            // mleft = M - 4 kq: accumulator (mt, r) is a row below M iff 16 mt + r < mleft

    // every thread of the workgroup; the caller's barrier follows
    static __device__ __forceinline__ void fill(const PfmHead &a, float *img, int tid, int nthr) {
        const int D = a.D, M = a.M;
        for (int i = tid; i < W_FLOATS; i += nthr) {
            const int tt = i & 3, l = (i >> 2) & 63, blk = i >> 8;
            const int j = 16 * (blk % MT) + (l & 15), m = 4 * (4 * (blk / MT) + tt) + (l >> 4);
            img[i] = (j < M && m < D) ? a.W[(size_t)j * D + m] : 0.f;
        }
        float *bi = img + W_FLOATS, *si = bi + ROW_FLOATS, *gi = si + ROW_FLOATS, *ei = gi + COL_FLOATS;
        for (int i = tid; i < ROW_FLOATS; i += nthr) {
            bi[i] = (i < M && a.b != nullptr) ? a.b[i] : 0.f;
            si[i] = i < M ? a.s[i] : 0.f;
        }
        for (int i = tid; i < COL_FLOATS; i += nthr) {
            const int m = 4 * (4 * (i >> 4) + (i & 3)) + ((i >> 2) & 3);       // (tq, kq, tt) -> column 4 (4 tq + tt) + kq
            gi[i] = (m < D && a.g != nullptr) ? a.g[m] : 0.f;
            ei[i] = (m < D && a.e != nullptr) ? a.e[m] : 0.f;
        }
    }

    __device__ __forceinline__ void init(const PfmHead &a, const float *img, const float *qrows, int l) {
        qi = reinterpret_cast<const f32x4 *>(qrows);
        lane = l;
        row = l & 15;
        kq = l >> 4;
        H = a.H;
        D = a.D;
        mleft = a.M - 4 * kq;
        wi = reinterpret_cast<const f32x4 *>(img);
        bi = reinterpret_cast<const f32x4 *>(img + W_FLOATS);
        si = reinterpret_cast<const f32x4 *>(img + W_FLOATS + ROW_FLOATS);
        gi = reinterpret_cast<const f32x4 *>(img + W_FLOATS + 2 * ROW_FLOATS);
        ei = reinterpret_cast<const f32x4 *>(img + W_FLOATS + 2 * ROW_FLOATS + COL_FLOATS);
    }

    // the column lane (., k) reads for MFMA step t, clamped into the row
    __device__ __forceinline__ int column(int t, int k) const {
        const int m = 4 * t + k;
        return m < D ? m : (D > 0 ? D - 1 : 0);
    }
    __device__ __forceinline__ int column(int t) const { return column(t, kq); }
    // kq, as a value the compiler knows nothing about.  Per slab: what is computed from it (KT clamped column offsets,
    // KT masks of the columns below D) is then computed where it is used -- a v_min, a v_cmp -- and not kept over the
    // candidate loop in registers that the loop does not have at KT = 32.
    __device__ __forceinline__ int kq_again() const {
        int k = kq;
        asm volatile("" : "+v"(k));
        return k;
    }

    // the query row `src` as the lane's B-fragment partners: q[.][4 t + kq], zero beyond D (and for a row that does not
    // exist: a product column then is 0 * c, and a NaN there is lost with the row's score)
    // (QLDS: into the wave's own LDS rows `qrows` instead, query s of the tile; wave_lds_fence() before the first read)
    __device__ __forceinline__ void query(const float *src, bool exists, float (&qf)[QR], float *qrows, int s) const {
        if constexpr (QLDS) {
            for (int i = lane; i < COL_FLOATS; i += 64) {
                const int m = 4 * (4 * (i >> 4) + (i & 3)) + ((i >> 2) & 3);   // (tq, kq, tt) -> column 4 (4 tq + tt) + kq
                qrows[s * COL_FLOATS + i] = (exists && m < D) ? src[m] : 0.f;
            }
            qf[0] = 0.f;
        } else {
#pragma unroll
            for (int t = 0; t < KT; ++t) qf[t] = 0.f;
            if (D > 0) {
#pragma unroll
                for (int t = 0; t < KT; ++t) qf[t] = src[column(t)];
            }
#pragma unroll
            for (int t = 0; t < KT; ++t) qf[t] = (exists && 4 * t + kq < D) ? qf[t] : 0.f;
        }
    }

    // what one group of four MFMA steps reads from LDS: a b128 per row tile, g and e, and (QLDS) a b128 per query
    struct Group {
        f32x4 w[MT], g, e, q[QLDS ? QT : 1];
    };
    __device__ __forceinline__ void read_group(int tq, Group &f) const {
        f.g = gi[4 * tq + kq];
        f.e = ei[4 * tq + kq];
        if constexpr (QLDS) {
#pragma unroll
            for (int s = 0; s < QT; ++s) f.q[s] = qi[(s * KG + tq) * 4 + kq];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) f.w[mt] = wi[(tq * MT + mt) * 64 + lane];
    }

    // x of one (query, step) -> the B operand, and the lane's share of the column sum
    static __device__ __forceinline__ float column_term(float xv, float gm, float em, float &vk) {
        vk = __builtin_fmaf(__builtin_fmaf(gm, xv, em), xv, vk);
        return xv;
    }

    // The slab's c registers against QT queries -> sv[s], the score of candidate `row` for query s (the same in all four
    // lanes of a candidate), without the query's bias.  The reads of group tq + 1 are issued before the MFMAs of group
    // tq and nothing is scheduled across a group's end, so a group waits (with a counted lgkmcnt) only for reads that had
    // a whole group of MFMAs to arrive, and no more than two groups' fragments are live.
    __device__ __forceinline__ void scores(const float (&bf)[KT], const float (&qf)[QT][QR], float cb, float (&sv)[QT]) const {
        f32x4 acc[QT][MT];
        float vk[QT];                                          // v_kq of this lane's column group
#pragma unroll
        for (int s = 0; s < QT; ++s) {
            vk[s] = 0.f;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[s][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        Group nxt;
        read_group(0, nxt);
        // every accumulator sees t ascending; the QT * MT chains are independent and interleave in the matrix pipe
#pragma unroll
        for (int tq = 0; tq < KG; ++tq) {
            const Group cur = nxt;
            if (tq + 1 < KG) read_group(tq + 1, nxt);
            f32x4 qv[QT];
#pragma unroll
            for (int s = 0; s < QT; ++s) {
                if constexpr (QLDS) {
                    qv[s] = cur.q[s];
                } else {
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt) qv[s][tt] = 4 * tq + tt < KT ? qf[s][4 * tq + tt] : 0.f;
                }
            }
            // the group's columns are 16 tq .. 16 tq + 15: all below H, all at or behind it (both wave-uniform), or the
            // one group that straddles H and selects per lane
            float x[QT][4];
            if (16 * tq + 16 <= H) {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    if (4 * tq + tt >= KT) continue;                           // (compile time)
#pragma unroll
                    for (int s = 0; s < QT; ++s)
                        x[s][tt] = column_term(__builtin_fmaxf(bf[4 * tq + tt] + qv[s][tt], 0.f), cur.g[tt], cur.e[tt], vk[s]);
                }
            } else if (16 * tq >= H) {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    if (4 * tq + tt >= KT) continue;
#pragma unroll
                    for (int s = 0; s < QT; ++s)
                        x[s][tt] = column_term(bf[4 * tq + tt] * qv[s][tt], cur.g[tt], cur.e[tt], vk[s]);
                }
            } else {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    if (4 * tq + tt >= KT) continue;
                    const bool relu = 4 * (4 * tq + tt) + kq < H;
#pragma unroll
                    for (int s = 0; s < QT; ++s) {
                        const float r = __builtin_fmaxf(bf[4 * tq + tt] + qv[s][tt], 0.f);
                        const float p = bf[4 * tq + tt] * qv[s][tt];
                        x[s][tt] = column_term(relu ? r : p, cur.g[tt], cur.e[tt], vk[s]);
                    }
                }
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    if (4 * tq + tt >= KT) continue;
#pragma unroll
                    for (int s = 0; s < QT; ++s)
                        acc[s][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.w[mt][tt], x[s][tt], acc[s][mt], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        float tk[QT];                                          // t_kq of this lane's row group
#pragma unroll
        for (int s = 0; s < QT; ++s) tk[s] = 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const f32x4 bv = bi[4 * mt + kq], sj = si[4 * mt + kq];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool below = 16 * mt + r < mleft;
#pragma unroll
                for (int s = 0; s < QT; ++s) {
                    const float y = (below ? acc[s][mt][r] : 0.f) + bv[r];
                    const float sy = sj[r] * y;
                    tk[s] = __builtin_fmaf(sy, y, tk[s]);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < QT; ++s) {
            float w = tk[s] + vk[s];
            w = w + __shfl_xor(w, 16);                         // (t_0 + v_0) + (t_1 + v_1) | (t_2 + v_2) + (t_3 + v_3)
            w = w + __shfl_xor(w, 32);
            sv[s] = w + cb;
        }
    }
};

// the B fragments of one slab in flight: c[slab + row][4 t + kq] and the row's bias
template <int KT>
struct PfmSlab {
    float bn[KT], cbn;

    __device__ __forceinline__ void clear() {
        cbn = 0.f;
#pragma unroll
        for (int t = 0; t < KT; ++t) bn[t] = 0.f;
    }
    // Unconditional loads from clamped addresses: a column past D reads column D - 1 and is zeroed in `take`, a row of
    // the NEXT chunk is read and ignored, a row past the table reads the table's last row.
    template <class Tile>
    __device__ __forceinline__ void load(const PfmHead &a, const Tile &wv, int kq, int64_t i) {
        const int64_t ic = i < a.n_c ? i : a.n_c - 1;
        const char *src = reinterpret_cast<const char *>(a.c + ic * a.c_stride);
        if (a.D > 0) {
#pragma unroll
            for (int t = 0; t < KT; ++t)                       // (one 64-bit row address and 32-bit column offsets)
                bn[t] = *reinterpret_cast<const float *>(src + (unsigned)(4 * wv.column(t, kq)));
        }
        if (a.c_bias != nullptr) cbn = a.c_bias[ic];
    }
    __device__ __forceinline__ void take(int D, int kq, float (&bf)[KT], float &cb) const {
        cb = cbn;
#pragma unroll
        for (int t = 0; t < KT; ++t) bf[t] = (4 * t + kq < D) ? bn[t] : 0.f;
    }
};

// Workgroup blockIdx.x = (group of tw tiles) x (group of PFM_WAVES / tw chunks of candidates), tw = 1, 2 or 4 (the host's
// pfm_tile_waves: with fewer than four tiles the waves share the head over neighbouring CHUNKS instead); consecutive
// workgroups are the tile groups of ONE chunk group.  -> the wave's own tile and chunk (ChunkGeom::tile / part may lie past
// the last one: pfm_idle)
__device__ __forceinline__ ChunkGeom pfm_geom(int64_t groups, int tw, int wave, int64_t chunk, int64_t n_c) {
    ChunkGeom g;
    g.tile = (blockIdx.x % groups) * tw + wave % tw;
    g.part = (blockIdx.x / groups) * (PFM_WAVES / tw) + wave / tw;
    g.first = g.tile * PFM_QT;
    g.c_begin = g.part * chunk;
    g.c_end = (g.c_begin + chunk < n_c) ? g.c_begin + chunk : n_c;
    return g;
}

inline int pfm_tile_waves(int64_t tiles) { return tiles >= 3 ? 4 : (int)tiles; }
// workgroups of a call over `tiles` tiles and `parts` chunks; *groups: the tile groups
inline int64_t pfm_grid(int64_t tiles, int64_t parts, int *tw, int64_t *groups) {
    *tw = pfm_tile_waves(tiles);
    *groups = cdiv(tiles, *tw);
    return *groups * cdiv(parts, PFM_WAVES / *tw);
}

struct PfmScanArgs {
    PfmHead h;
    const int64_t *excl_off, *excl_ids;
    float *out_scores;        // [n_q, parts, K]
    int64_t *out_ids;
    int64_t n_q, chunk, parts, tiles, groups;
    int K, tw;
};

template <int KT, int MT>
__global__ __launch_bounds__(64 * PFM_WAVES) void pfm_scan_kernel(PfmScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfm_lds[];
    typedef PfmTile<KT, MT> Tile;
    constexpr int QT = PFM_QT;
    const int K = a.K, D = a.h.D;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *img = reinterpret_cast<float *>(pfm_lds);
    float *qrows = img + Tile::HEAD_FLOATS + wave * Tile::Q_FLOATS;           // this wave's query rows (QLDS)
    float *sc = img + Tile::HEAD_FLOATS + PFM_WAVES * Tile::Q_FLOATS + wave * (2 * QT * K);    // [QT][K], this wave's
    int *id = reinterpret_cast<int *>(sc + QT * K);            // [QT][K]  candidate - chunk begin

    Tile::fill(a.h, img, threadIdx.x, 64 * PFM_WAVES);
    for (int i = lane; i < QT * K; i += 64) { sc[i] = -INFINITY; id[i] = fill_id<int>::value; }
    __syncthreads();

    const ChunkGeom g = pfm_geom(a.groups, a.tw, wave, a.chunk, a.h.n_c);
    if (g.tile >= a.tiles || g.part >= a.parts) return;        // (wave-uniform; no barrier follows)
    const int64_t u0 = g.first, c_begin = g.c_begin, c_end = g.c_end;

    Tile wv;
    wv.init(a.h, img, qrows, lane);
    const int row = wv.row, kq = wv.kq;
    float qf[QT][Tile::QR], qb[QT], thr[QT];                   // qb, thr: wave-uniform
#pragma unroll
    for (int s = 0; s < QT; ++s) {
        const int64_t u = u0 + s;
        const bool exists = u < a.n_q;
        const int64_t uc = exists ? u : a.n_q - 1;
        wv.query(a.h.q + uc * D, exists, qf[s], qrows, s);
        qb[s] = a.h.q_bias != nullptr ? a.h.q_bias[uc] : 0.f;
        thr[s] = exists ? -INFINITY : INFINITY;                // rows past n_q never survive
    }
    wave_lds_fence();

    PfmSlab<KT> nx;
    float bf[KT], cb;
    nx.clear();
    nx.take(D, kq, bf, cb);
    // (the trip before c_begin only loads the first slab: the loads have ONE site)
    for (int64_t base = c_begin - 16; base < c_end; base += 16) {
        const int kv = wv.kq_again();
        if (base + 16 < c_end) nx.load(a.h, wv, kv, base + 16 + row);
        if (base < c_begin) {
            nx.take(D, kv, bf, cb);
            continue;
        }
        float sv[QT];
        wv.scores(bf, qf, cb, sv);
        const bool live = kq == 0 && base + row < c_end;       // one lane per candidate offers it
        bool any = false;
#pragma unroll
        for (int s = 0; s < QT; ++s) {
            sv[s] = sv[s] + qb[s];
            any |= live && sv[s] > thr[s];                     // (false for a NaN score)
        }
        if (__ballot(any) != 0) {
            // survivors, one at a time (wave-uniform control flow from here on)
#pragma unroll
            for (int s = 0; s < QT; ++s) {
                unsigned long long m = __ballot(live && sv[s] > thr[s]);
                while (m) {
                    const int src = __builtin_ctzll(m);
                    m &= m - 1;
                    const float v = lane_value(sv[s], src);
                    const int64_t ci = base + src;             // (src < 16: a lane of kq == 0)
                    if (!(v > thr[s])) continue;               // (an earlier survivor raised the bar)
                    if (is_excluded(a.excl_off, a.excl_ids, u0 + s, ci)) continue;
                    thr[s] = list_insert<int>(sc + s * K, id + s * K, K, v, (int)(ci - c_begin), lane);
                }
            }
        }
        nx.take(D, kv, bf, cb);
    }

    // the partial lists, filled up with (-inf, -1)
    for (int ql = 0; ql < QT; ++ql) {
        const int64_t u = u0 + ql;
        if (u >= a.n_q) break;
        const int64_t o = (u * a.parts + g.part) * K;
        for (int p = lane; p < K; p += 64) {
            const int ci = id[ql * K + p];
            a.out_scores[o + p] = sc[ql * K + p];              // (-inf in an unused slot)
            a.out_ids[o + p] = ci != fill_id<int>::value ? c_begin + ci : (int64_t)-1;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// r4r_rank_pfm: r4r_rank_dot's three launches over this file's chain (A and C: topk_device.h's scalar kernels over
// PfmHead); B, rank_pfm_scan_kernel, is the scan's stream over tiles of QT PAIRS (query rows gathered through q_idx) with
// counters in place of lists and one 64-bit integer atomic per (pair, chunk).
struct PfmRankArgs {
    PfmHead h;
    const int64_t *q_idx, *t_idx;
    const float *t_score;     // out_score, written by launch A
    int64_t *out_rank;
    int64_t n_p, chunk, parts, tiles, groups;
    int tw;
};

template <int KT, int MT>
__global__ __launch_bounds__(64 * PFM_WAVES) void rank_pfm_scan_kernel(PfmRankArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pfm_lds[];
    typedef PfmTile<KT, MT> Tile;
    constexpr int PT = PFM_QT;
    const int D = a.h.D;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *img = reinterpret_cast<float *>(pfm_lds);
    float *qrows = img + Tile::HEAD_FLOATS + wave * Tile::Q_FLOATS;           // this wave's query rows (QLDS)

    Tile::fill(a.h, img, threadIdx.x, 64 * PFM_WAVES);
    __syncthreads();

    const ChunkGeom g = pfm_geom(a.groups, a.tw, wave, a.chunk, a.h.n_c);
    if (g.tile >= a.tiles || g.part >= a.parts) return;        // (wave-uniform; no barrier follows)
    const int64_t p0 = g.first, c_begin = g.c_begin, c_end = g.c_end;
    const int c_len = g.c_len();

    Tile wv;
    wv.init(a.h, img, qrows, lane);
    const int row = wv.row, kq = wv.kq;
    // Of each pair: its query row, its query bias, its target's score and its target's id relative to the chunk (-1:
    // before it, so no tie is ahead; INT_MAX: behind it, so every tie is).  A pair past n_p or at -1 waits for a score
    // above +inf: it counts nothing.  (All wave-uniform.)
    float qf[PT][Tile::QR], qb[PT], ts[PT];
    int trel[PT], cnt[PT];
#pragma unroll
    for (int s = 0; s < PT; ++s) {
        const int64_t p = p0 + s;
        const bool exists = p < a.n_p;
        const int64_t pc = exists ? p : a.n_p - 1;
        const int64_t u = a.q_idx[pc];
        wv.query(a.h.q + u * D, exists, qf[s], qrows, s);
        qb[s] = a.h.q_bias != nullptr ? a.h.q_bias[u] : 0.f;
        const float st = a.t_score[pc];
        const int64_t d = a.t_idx[pc] - c_begin;
        const bool ranked = exists && st > -INFINITY;          // (false for NaN)
        ts[s] = ranked ? st : INFINITY;
        trel[s] = !ranked || d < 0 ? -1 : (d > 0x7fffffff ? 0x7fffffff : (int)d);
        cnt[s] = 0;
    }
    wave_lds_fence();

    PfmSlab<KT> nx;
    float bf[KT], cb;
    nx.clear();
    nx.take(D, kq, bf, cb);
    // (the trip before c_begin only loads the first slab: the loads have ONE site)
    for (int64_t base = c_begin - 16; base < c_end; base += 16) {
        const int kv = wv.kq_again();
        if (base + 16 < c_end) nx.load(a.h, wv, kv, base + 16 + row);
        if (base < c_begin) {
            nx.take(D, kv, bf, cb);
            continue;
        }
        float sv[PT];
        wv.scores(bf, qf, cb, sv);
        const int rel = (int)(base - c_begin) + row;
        const bool live = kq == 0 && rel < c_len;              // one lane per candidate counts it
#pragma unroll
        for (int s = 0; s < PT; ++s)
            cnt[s] += (live && ahead<int>(sv[s] + qb[s], rel, ts[s], trel[s])) ? 1 : 0;     // (false for a NaN score)
        nx.take(D, kv, bf, cb);
    }

    // lane s adds pair s's count over the wave to its rank -- one atomic instruction per wave
    int mine = 0;
#pragma unroll
    for (int s = 0; s < PT; ++s) {
        int v = cnt[s];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
        if (lane == s) mine = v;
    }
    // (mine > 0 only for a pair below n_p whose target is ranked: the others wait for +inf)
    if (lane < PT && mine > 0)
        atomicAdd(reinterpret_cast<unsigned long long *>(a.out_rank + p0 + lane), (unsigned long long)mine);
}

// The dynamic LDS of a launch: the head's image, the four waves' query rows (QLDS) and, for the list scan, their lists
template <int KT, int MT>
constexpr size_t pfm_scan_lds(int K) {
    return (size_t)(PfmTile<KT, MT>::HEAD_FLOATS + PFM_WAVES * PfmTile<KT, MT>::Q_FLOATS) * 4 +
           (size_t)PFM_WAVES * PFM_QT * (size_t)K * 8;
}
template <int KT, int MT>
constexpr size_t pfm_rank_lds() { return (size_t)(PfmTile<KT, MT>::HEAD_FLOATS + PFM_WAVES * PfmTile<KT, MT>::Q_FLOATS) * 4; }

// A kernel whose launches may ask for more dynamic LDS than PFM_STATIC_LDS needs its attribute raised first -- to the
// most any launch of it asks for (`most`), once per device: `raised` is the instantiation's flag per device ordinal (the
// attribute belongs to the device's copy of the code object; a device past the flags is raised at every call).  Called
// before the FIRST launch of an entry point: where the runtime refuses, the call returns and has launched nothing.
constexpr int PFM_DEVICES = 64;
int pfm_allow_lds(const void *kernel, size_t most, const char *what, unsigned char *raised) {
    if (most <= PFM_STATIC_LDS) return R4R_OK;
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev >= 0 && dev < PFM_DEVICES && raised[dev]) return R4R_OK;
    if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: %zu bytes of LDS refused: %s", what, most, hipGetErrorString(e));
        return R4R_ERR_LAUNCH;
    }
    if (dev < PFM_DEVICES) raised[dev] = 1;
    return R4R_OK;
}

template <int KT, int MT>
int allow_pfm_scan() {
    static unsigned char raised[PFM_DEVICES];
    return pfm_allow_lds(reinterpret_cast<const void *>(&pfm_scan_kernel<KT, MT>), pfm_scan_lds<KT, MT>(TOPK_MAX_K),
                         "pfm_scan_kernel", raised);
}
template <int KT, int MT>
int allow_pfm_rank() {
    static unsigned char raised[PFM_DEVICES];
    return pfm_allow_lds(reinterpret_cast<const void *>(&rank_pfm_scan_kernel<KT, MT>), pfm_rank_lds<KT, MT>(),
                         "rank_pfm_scan_kernel", raised);
}

// (the entry point has called allow_pfm_scan / allow_pfm_rank of the same class)
template <int KT, int MT>
int launch_pfm_scan(const PfmScanArgs &a, int64_t grid, hipStream_t st) {
    const size_t lds = pfm_scan_lds<KT, MT>(a.K);
    hipLaunchKernelGGL((pfm_scan_kernel<KT, MT>), dim3((unsigned)grid), dim3(64 * PFM_WAVES), lds, st, a);
    return check_launch("pfm_scan_kernel");
}

template <int KT, int MT>
int launch_pfm_rank(const PfmRankArgs &a, int64_t grid, hipStream_t st) {
    const size_t lds = pfm_rank_lds<KT, MT>();
    hipLaunchKernelGGL((rank_pfm_scan_kernel<KT, MT>), dim3((unsigned)grid), dim3(64 * PFM_WAVES), lds, st, a);
    return check_launch("rank_pfm_scan_kernel");
}

// Five classes <KT, MT>, the smallest that holds BOTH D <= 4 KT and M <= 16 MT: <3, 1> <4, 1> <8, 2> <16, 4> <32, 8>.
// MF (H = G = L, M = 2 L) at latent sizes 6 / 8 / 16 / 32 / 64 lands on each of them exactly; every other width runs
// zero steps and zero rows up to its class (latent size 10: 5 of 8 steps, 2 of 2 tiles).
inline int pfm_class(int D, int M) {
    return (D <= 12 && M <= 16) ? 0 : (D <= 16 && M <= 16) ? 1 : (D <= 32 && M <= 32) ? 2 : (D <= 64 && M <= 64) ? 3 : 4;
}

#define PFM_DISPATCH(FN, D, M, ...)                        \
    do {                                                   \
        switch (pfm_class(D, M)) {                         \
        case 0: return FN<3, 1>(__VA_ARGS__);              \
        case 1: return FN<4, 1>(__VA_ARGS__);              \
        case 2: return FN<8, 2>(__VA_ARGS__);              \
        case 3: return FN<16, 4>(__VA_ARGS__);             \
        default: return FN<32, 8>(__VA_ARGS__);            \
        }                                                  \
    } while (0)

int dispatch_pfm_scan(const PfmScanArgs &a, int64_t grid, hipStream_t st) {
    PFM_DISPATCH(launch_pfm_scan, a.h.D, a.h.M, a, grid, st);
}
int dispatch_pfm_rank(const PfmRankArgs &a, int64_t grid, hipStream_t st) {
    PFM_DISPATCH(launch_pfm_rank, a.h.D, a.h.M, a, grid, st);
}
int dispatch_pfm_allow_scan(int D, int M) { PFM_DISPATCH(allow_pfm_scan, D, M); }
int dispatch_pfm_allow_rank(int D, int M) { PFM_DISPATCH(allow_pfm_rank, D, M); }

inline PfmHead pfm_head(const float *q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                        const float *c_bias, const float *W, const float *b, const float *s, const float *g, const float *e,
                        int H, int G, int M) {
    PfmHead h;
    h.q = q; h.q_bias = q_bias; h.c = c; h.c_bias = c_bias; h.W = W; h.b = b; h.s = s; h.g = g; h.e = e;
    h.n_c = n_c; h.c_stride = c_stride; h.H = H; h.G = G; h.M = M;
    // (out-of-range H or G: ranges() refuses before D is used)
    h.D = (H >= 0 && H <= PFM_MAX_H && G >= 0 && G <= PFM_MAX_G) ? H + G : 0;
    return h;
}

}  // namespace
}  // namespace r4r

using namespace r4r;

extern "C" size_t r4r_topk_pfm_ws_bytes(int64_t n_q, int64_t n_c, int K, int64_t chunk) {
    return lists_ws_bytes(n_q, n_c, K, chunk, PFM_QT);
}

extern "C" int r4r_topk_pfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                            const float *c_bias, const float *W, const float *b, const float *s, const float *g,
                            const float *e, int H, int G, int M, const int64_t *excl_off, const int64_t *excl_ids, int K,
                            int64_t chunk, void *ws, size_t ws_bytes, int64_t *out_ids, float *out_scores, void *stream) {
    PfmScanArgs a;
    a.h = pfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, g, e, H, G, M);
    bool work;
    int rc = topk_check("topk_pfm", a.h, n_q, excl_off, excl_ids, K, chunk, out_ids, out_scores, &work);
    if (rc != R4R_OK || !work) return rc;
    ListsPlan p;
    rc = topk_plan("topk_pfm", n_q, n_c, K, chunk, PFM_QT, PFM_QT, ws, ws_bytes, out_ids, out_scores, &p);
    if (rc != R4R_OK) return rc;
    a.excl_off = excl_off; a.excl_ids = excl_ids;
    a.out_scores = p.scan_scores; a.out_ids = p.scan_ids;
    a.n_q = n_q; a.chunk = p.chunk; a.parts = p.parts; a.tiles = p.tiles; a.K = K;
    const int64_t grid = pfm_grid(p.tiles, p.parts, &a.tw, &a.groups);
    rc = dispatch_pfm_allow_scan(a.h.D, M);                    // before the first launch
    if (rc != R4R_OK) return rc;
    hipStream_t st = as_stream(stream);
    return topk_finish(p, dispatch_pfm_scan(a, grid, st), n_q, K, out_ids, out_scores, st);
}

extern "C" int r4r_pair_pfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                            const float *c_bias, const float *W, const float *b, const float *s, const float *g,
                            const float *e, int H, int G, int M, const int64_t *q_idx, const int64_t *c_idx, int64_t n,
                            float *out, void *stream) {
    const PfmHead h = pfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, g, e, H, G, M);
    bool work;
    const int rc = pair_check("pair_pfm", h, n_q, q_idx, c_idx, n, out, &work);
    if (rc != R4R_OK || !work) return rc;
    return launch_pairs(h, q_idx, c_idx, n, out, as_stream(stream));
}

extern "C" int r4r_rank_pfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                            const float *c_bias, const float *W, const float *b, const float *s, const float *g,
                            const float *e, int H, int G, int M, const int64_t *q_idx, const int64_t *t_idx, int64_t n_p,
                            const int64_t *excl_off, const int64_t *excl_ids, int64_t chunk, int64_t *out_rank,
                            float *out_score, void *stream) {
    PfmRankArgs a;
    a.h = pfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, g, e, H, G, M);
    bool work;
    int rc = rank_check("rank_pfm", a.h, n_q, q_idx, t_idx, n_p, excl_off, excl_ids, chunk, out_rank, out_score, &work);
    if (rc != R4R_OK || !work) return rc;
    ChunkPlan p;
    rc = rank_plan("rank_pfm", n_p, n_c, chunk, PFM_QT, PFM_QT, &p);
    if (rc != R4R_OK) return rc;
    a.q_idx = q_idx; a.t_idx = t_idx;
    a.t_score = out_score; a.out_rank = out_rank;
    a.n_p = n_p; a.chunk = p.chunk; a.parts = p.parts; a.tiles = p.tiles;
    const int64_t grid = pfm_grid(p.tiles, p.parts, &a.tw, &a.groups);
    rc = dispatch_pfm_allow_rank(a.h.D, M);                    // before the first launch: the targets' is not the scan's
    if (rc != R4R_OK) return rc;
    hipStream_t st = as_stream(stream);
    rc = launch_rank_targets(a.h, q_idx, t_idx, n_p, out_score, out_rank, st);
    if (rc != R4R_OK) return rc;
    return rank_finish(a.h, dispatch_pfm_rank(a, grid, st), q_idx, t_idx, n_p, excl_off, excl_ids, out_score, out_rank, st);
}

// Slates (slate_device.h): the K best of, and the place of a target among, per-query candidate lists
extern "C" int r4r_slate_topk_pfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c,
                                  int64_t c_stride, const float *c_bias, const float *W, const float *b, const float *s,
                                  const float *g, const float *e, int H, int G, int M, const int64_t *q_idx,
                                  const int64_t *slate_off, const int64_t *slate_ids, int64_t n_s, int64_t max_len,
                                  const int64_t *excl_off, const int64_t *excl_ids, int K, void *ws, size_t ws_bytes,
                                  int64_t *out_ids, float *out_scores, void *stream) {
    const PfmHead h = pfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, g, e, H, G, M);
    return slate_topk_call("slate_topk_pfm", h, n_q, q_idx, slate_off, slate_ids, n_s, max_len, excl_off, excl_ids, K,
                           ws, ws_bytes, out_ids, out_scores, stream);
}

extern "C" int r4r_slate_rank_pfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c,
                                  int64_t c_stride, const float *c_bias, const float *W, const float *b, const float *s,
                                  const float *g, const float *e, int H, int G, int M, const int64_t *q_idx,
                                  const int64_t *t_idx, const int64_t *slate_off, const int64_t *slate_ids, int64_t n_p,
                                  int64_t max_len, const int64_t *excl_off, const int64_t *excl_ids, int64_t *out_rank,
                                  float *out_score, void *stream) {
    const PfmHead h = pfm_head(q, q_bias, c, n_c, c_stride, c_bias, W, b, s, g, e, H, G, M);
    return slate_rank_call("slate_rank_pfm", h, n_q, q_idx, t_idx, slate_off, slate_ids, n_p, max_len, excl_off,
                           excl_ids, out_rank, out_score, stream);
}

// What-if documents (include/r4r.h, "What-if documents"): the single-document families' tower over VARIANTS of their
// owners' documents -- chosen reviews taken away, chosen positions occluded -- built on the device from the HBM-resident
// token pools and enqueued from C.
//
// r4r_tower_span_variants is r4r_tower_span_fwd (tower_span.hip) at R = 0 with r4r_tower_build_variants in
// r4r_tower_build's place in every round: the same r4r_textcnn_fwd and r4r_linear_fwd calls over the same workspace
// layout, so with nothing removed the latents keep their bits (tests/test_gpu_tower_variants_span.py).
//
// The kernels of this file are the masked builder -- one workgroup per row, docs_masked_device.h's writer; integer work,
// bound by its int64 output like r4r_tower_build -- and a word copy that hands a round's pooled / argmax to the caller.
#include "common.h"
#include "docs_masked_device.h"

namespace r4r {

struct VariantBuildArgs {
    const int32_t *tok, *occ_pos;
    const int64_t *rev_off, *first, *ids, *drop, *occ_off;
    int64_t owners;
    int64_t *docs;
    int T;
};

// grid (n): row r = owner ids[r] minus the reviews of drop[r], the positions of occ_off[r] .. occ_off[r + 1] zeroed; an
// id outside [0, owners) has no reviews (rb = re = 0: a zero document), so nothing is read past the pool whatever the
// ids hold.
__global__ void __launch_bounds__(256) tower_build_variants_kernel(const VariantBuildArgs a) {
    __shared__ MaskedDocLds lds;
    const int64_t row = blockIdx.x;
    const int64_t id = a.ids[row];
    const bool known = id >= 0 && id < a.owners;
    const int64_t rb = known ? a.first[id] : 0, re = known ? a.first[id + 1] : 0;
    const uint64_t drop = a.drop ? (uint64_t)a.drop[row] : 0;
    int64_t ob = 0, oe = 0;
    if (a.occ_off) {
        ob = a.occ_off[row];
        oe = a.occ_off[row + 1];
    }
    write_doc_masked(a.tok, a.rev_off, rb, re, drop, a.occ_pos + ob, oe > ob ? oe - ob : 0, a.T,
                     a.docs + row * (int64_t)a.T, lds);
}

// dst[i] = src[i] over n 4-byte words (a round's pooled / argmax out of the workspace)
__global__ void __launch_bounds__(256) copy_words_kernel(const uint32_t *src, uint32_t *dst, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

static int copy_words(const void *src, void *dst, int64_t n, void *stream) {
    const int64_t blocks = cdiv(n, 256);
    hipLaunchKernelGGL(copy_words_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                       as_stream(stream), static_cast<const uint32_t *>(src), static_cast<uint32_t *>(dst), n);
    return check_launch("r4r_tower_span_variants");
}

static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// r4r_tower_span_fwd's workspace at R = 0: documents, pooled, argmax, the conv's own workspace
struct VariantWs {
    size_t docs, pooled, argmax, conv;
    size_t total() const { return docs + pooled + argmax + conv; }
};

static VariantWs variant_ws(int64_t rows, int T, int E, int F, int64_t V) {
    VariantWs w;
    w.docs = align256((size_t)rows * T * 8);
    w.pooled = align256((size_t)rows * F * 4);
    w.argmax = align256((size_t)rows * F * 4);
    w.conv = align256(r4r_textcnn_ws_bytes(rows, T, E, F, V));
    return w;
}

static int check_variant_shape(const char *who, int64_t owners, int64_t n, int T, const void *occ_off,
                               const void *occ_pos) {
    R4R_REQUIRE(n > 0 && n < (1ll << 31) && owners >= 0, "%s: bad shape n=%lld owners=%lld", who, (long long)n,
                (long long)owners);
    R4R_REQUIRE(T >= 1 && T <= VARIANT_MAX_T, "%s: T=%d outside 1 .. %d (one occlusion flag per position)", who, T,
                VARIANT_MAX_T);
    R4R_REQUIRE(!occ_off || occ_pos, "%s: occ_off without occ_pos", who);
    return R4R_OK;
}

}  // namespace r4r

using namespace r4r;

extern "C" int r4r_tower_build_variants(const int32_t *tok, const int64_t *rev_off, const int64_t *first,
                                        int64_t owners, const int64_t *ids, const int64_t *drop,
                                        const int64_t *occ_off, const int32_t *occ_pos, int64_t n, int T, int64_t *docs,
                                        void *stream) {
    if (n == 0) return R4R_OK;
    R4R_REQUIRE(tok && rev_off && first && ids && docs, "r4r_tower_build_variants: null pointer");
    if (int rc = check_variant_shape("r4r_tower_build_variants", owners, n, T, occ_off, occ_pos)) return rc;
    VariantBuildArgs a;
    a.tok = tok; a.occ_pos = occ_pos; a.rev_off = rev_off; a.first = first; a.ids = ids; a.drop = drop;
    a.occ_off = occ_off; a.owners = owners; a.docs = docs; a.T = T;
    hipLaunchKernelGGL(tower_build_variants_kernel, dim3((unsigned)n), dim3(256), 0, as_stream(stream), a);
    return check_launch("r4r_tower_build_variants");
}

extern "C" size_t r4r_tower_span_variants_ws_bytes(int64_t group, int T, int E, int F, int L, int64_t V) {
    if (group < 1 || group >= (1ll << 31) || T < 1 || T > VARIANT_MAX_T || E <= 0 || F <= 0 || L <= 0 || V <= 0) return 0;
    return variant_ws(group, T, E, F, V).total();
}

extern "C" int r4r_tower_span_variants(const int32_t *tok, const int64_t *rev_off, const int64_t *first,
                                       int64_t owners, const int64_t *ids, const int64_t *drop,
                                       const int64_t *occ_off, const int32_t *occ_pos, int64_t n, int64_t group, int T,
                                       const float *table, int64_t V, const float *conv_w, const float *conv_b,
                                       const float *fc_w, const float *fc_b, int E, int F, int L, float *latent,
                                       float *pooled_out, int32_t *argmax_out, void *ws, size_t ws_bytes,
                                       int64_t *groups_done, void *stream) {
    if (groups_done) *groups_done = 0;
    if (n == 0) return R4R_OK;
    // ---- everything that can be refused, before the first launch
    R4R_REQUIRE(tok && rev_off && first && ids && table && conv_w && conv_b && fc_w && fc_b && latent && ws,
                "r4r_tower_span_variants: null pointer");
    if (int rc = check_variant_shape("r4r_tower_span_variants", owners, n, T, occ_off, occ_pos)) return rc;
    R4R_REQUIRE(group >= 1, "r4r_tower_span_variants: group = %lld rows per round, at least 1", (long long)group);
    R4R_REQUIRE(E > 0 && E % 4 == 0, "r4r_tower_span_variants: word_embed_size %d must be a positive multiple of 4 (pad "
                                     "the frozen table and the conv weight on the host otherwise)", E);
    R4R_REQUIRE(F > 0 && F <= 112, "r4r_tower_span_variants: %d filters > 112 supported", F);
    R4R_REQUIRE(L > 0 && V > 0, "r4r_tower_span_variants: bad sizes L=%d V=%lld", L, (long long)V);
    const int64_t G = group < n ? group : n;                // rows of the largest round
    R4R_REQUIRE(G * (int64_t)((T + 2 + 127) / 128) < (1ll << 31),
                "r4r_tower_span_variants: %lld rows of %d words per round: the conv's grid is too large", (long long)G, T);
    // r4r_tower_span_fwd's layout: the largest round's, the conv's part sized for a smaller last round too
    const VariantWs use = variant_ws(G, T, E, F, V);
    const int64_t tail = n % G;
    const size_t tail_conv = tail ? r4r_textcnn_ws_bytes(tail, T, E, F, V) : 0;
    const size_t want = use.total() - use.conv + (tail_conv > use.conv ? tail_conv : use.conv);
    if (ws_bytes < want) {
        set_error("r4r_tower_span_variants: workspace %zu < %zu bytes (r4r_tower_span_variants_ws_bytes)", ws_bytes, want);
        return R4R_ERR_WORKSPACE;
    }
    const size_t conv_bytes = ws_bytes - (use.total() - use.conv);
    char *base = static_cast<char *>(ws);
    int64_t *docs = reinterpret_cast<int64_t *>(base);
    float *pooled = reinterpret_cast<float *>(base + use.docs);
    int32_t *argmax = reinterpret_cast<int32_t *>(base + use.docs + use.pooled);
    void *conv_ws = base + use.docs + use.pooled + use.argmax;
    // ---- round g: rows [g group, min(n, (g + 1) group)); the ONE stream orders the workspace's reuse.  occ_off's
    // entries index occ_pos absolutely, so the round's slice of it serves as it stands.
    for (int64_t g = 0, at = 0; at < n; ++g, at += G) {
        const int64_t m = n - at < G ? n - at : G;
        if (int rc = r4r_tower_build_variants(tok, rev_off, first, owners, ids + at, drop ? drop + at : nullptr,
                                              occ_off ? occ_off + at : nullptr, occ_pos, m, T, docs, stream))
            return rc;
        if (int rc = r4r_textcnn_fwd(table, V, docs, conv_w, conv_b, pooled, argmax, conv_ws, conv_bytes, m, T, E, F, stream))
            return rc;
        if (int rc = r4r_linear_fwd(pooled, fc_w, fc_b, latent + at * (int64_t)L, m, F, L, 0, stream)) return rc;
        if (pooled_out)
            if (int rc = copy_words(pooled, pooled_out + at * (int64_t)F, m * (int64_t)F, stream)) return rc;
        if (argmax_out)
            if (int rc = copy_words(argmax, argmax_out + at * (int64_t)F, m * (int64_t)F, stream)) return rc;
        if (groups_done) *groups_done = g + 1;
    }
    return R4R_OK;
}

// Tower spans (include/r4r.h, "Tower spans"): one side's TextCNN tower over a list of owners -- every eligible item at a
// catalogue refresh, every requested user at a recommend / rank call -- with the documents built on the device from the
// HBM-resident token pools and every launch enqueued from C.
//
// Replaces the host side of reviews4rec_amd/recommend.py's catalogue passes: _documents / _attended (numpy over
// data._np_docs / _np_reviews / _np_neighbours, one [n, T] int64 block copied to the device per tower_batch owners) and
// the per-chunk Python calls of _tower.  Round g is the chunk the host path forms, so its three launches --
// r4r_tower_build, r4r_textcnn_fwd, r4r_linear_fwd -- see the rows, the N (hence the conv algorithm) and the arguments
// the per-chunk calls see: the latents keep their bits (tests/test_gpu_tower_span.py).
//
// The only kernel of this file is the builder: one workgroup per owner, the row writers of docs_device.h with nothing
// removed (skip = -1).  Integer work, bound by its int64 output like r4r_batch_build.
#include "common.h"
#include "docs_device.h"

namespace r4r {

struct TowerBuildArgs {
    const int32_t *tok;
    const int64_t *rev_off, *first, *nb, *ids;
    int64_t owners, pad;
    int64_t *docs, *neigh;
    int T, R, W;
};

// grid (n): row r = owner ids[r]; an id outside [0, owners) has no reviews (rb = re = 0: a zero document, pad
// neighbours), so nothing is read past the pool whatever the ids hold.
__global__ void __launch_bounds__(256) tower_build_kernel(const TowerBuildArgs a) {
    const int64_t row = blockIdx.x;
    const int64_t id = a.ids[row];
    const bool known = id >= 0 && id < a.owners;
    const int64_t rb = known ? a.first[id] : 0, re = known ? a.first[id + 1] : 0;
    if (a.R > 0) {
        write_reviews(a.tok, a.rev_off, rb, re, -1, a.R, a.W, a.docs + row * ((int64_t)a.R * a.W));
        write_neighbours(a.nb, rb, a.nb ? re : rb, -1, a.pad, a.neigh + row * NEIGHBOURS);   // (no nb: a pool without a review)
    } else {
        write_doc(a.tok, a.rev_off, rb, re, -1, a.T, a.docs + row * (int64_t)a.T);
    }
}

static inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

static int check_build_shape(const char *who, int64_t owners, int64_t n, int T, int R, int W) {
    R4R_REQUIRE(n > 0 && n < (1ll << 31) && owners >= 0 &&
                    ((R > 0 && W > 0 && (int64_t)R * W < (1ll << 31)) || (R == 0 && T > 0)),
                "%s: bad shape n=%lld owners=%lld T=%d R=%d W=%d", who, (long long)n, (long long)owners, T, R, W);
    return R4R_OK;
}

// the parts of one group's workspace, in order: documents, pooled, argmax, the conv's own workspace
struct TowerWs {
    size_t docs, pooled, argmax, conv;
    size_t total() const { return docs + pooled + argmax + conv; }
};

static TowerWs tower_ws(int64_t rows, int width, int E, int F, int64_t V) {
    TowerWs w;
    w.docs = align256((size_t)rows * width * 8);
    w.pooled = align256((size_t)rows * F * 4);
    w.argmax = align256((size_t)rows * F * 4);
    w.conv = align256(r4r_textcnn_ws_bytes(rows, width, E, F, V));
    return w;
}

}  // namespace r4r

using namespace r4r;

extern "C" int r4r_tower_build(const int32_t *tok, const int64_t *rev_off, const int64_t *first, const int64_t *nb,
                               int64_t owners, const int64_t *ids, int64_t n, int T, int R, int W, int64_t pad,
                               int64_t *docs, int64_t *neigh, void *stream) {
    if (n == 0) return R4R_OK;
    R4R_REQUIRE(tok && rev_off && first && ids && docs && (R <= 0 || neigh), "r4r_tower_build: null pointer");
    if (int rc = check_build_shape("r4r_tower_build", owners, n, T, R, W)) return rc;
    TowerBuildArgs a;
    a.tok = tok; a.rev_off = rev_off; a.first = first; a.nb = nb; a.ids = ids;
    a.owners = owners; a.pad = pad; a.docs = docs; a.neigh = neigh; a.T = T; a.R = R; a.W = W;
    hipLaunchKernelGGL(tower_build_kernel, dim3((unsigned)n), dim3(256), 0, as_stream(stream), a);
    return check_launch("r4r_tower_build");
}

extern "C" size_t r4r_tower_span_ws_bytes(int64_t group, int T, int R, int W, int E, int F, int L, int64_t V) {
    if (group < 1 || group >= (1ll << 31) || R < 0 || (R > 0 ? W <= 0 : T <= 0) || E <= 0 || F <= 0 || L <= 0 || V <= 0)
        return 0;
    const int64_t rows = group * (R > 0 ? R : 1);
    if (rows >= (1ll << 31)) return 0;
    return tower_ws(rows, R > 0 ? W : T, E, F, V).total();
}

extern "C" int r4r_tower_span_fwd(const int32_t *tok, const int64_t *rev_off, const int64_t *first, const int64_t *nb,
                              int64_t owners, const int64_t *ids, int64_t n, int64_t group, int T, int R, int W,
                              int64_t pad, const float *table, int64_t V, const float *conv_w, const float *conv_b,
                              const float *fc_w, const float *fc_b, int E, int F, int L, float *latent,
                              int64_t *neigh, void *ws, size_t ws_bytes, int64_t *groups_done, void *stream) {
    if (groups_done) *groups_done = 0;
    if (n == 0) return R4R_OK;
    // ---- everything that can be refused, before the first launch
    R4R_REQUIRE(tok && rev_off && first && ids && table && conv_w && conv_b && fc_w && fc_b && latent && ws &&
                    (R <= 0 || neigh),
                "r4r_tower_span_fwd: null pointer");
    R4R_REQUIRE(group >= 1, "r4r_tower_span_fwd: group = %lld owners per round, at least 1", (long long)group);
    if (int rc = check_build_shape("r4r_tower_span_fwd", owners, n, T, R, W)) return rc;
    R4R_REQUIRE(E > 0 && E % 4 == 0, "r4r_tower_span_fwd: word_embed_size %d must be a positive multiple of 4 (pad the "
                                     "frozen table and the conv weight on the host otherwise)", E);
    R4R_REQUIRE(F > 0 && F <= 112, "r4r_tower_span_fwd: %d filters > 112 supported", F);
    R4R_REQUIRE(L > 0 && V > 0, "r4r_tower_span_fwd: bad sizes L=%d V=%lld", L, (long long)V);
    const int per = R > 0 ? R : 1, width = R > 0 ? W : T;
    const int64_t G = group < n ? group : n;                // owners of the largest round
    const int64_t rows_max = G * per;
    R4R_REQUIRE(rows_max * (int64_t)((width + 2 + 127) / 128) < (1ll << 31),
                "r4r_tower_span_fwd: %lld rows of %d words per round: the conv's grid is too large", (long long)rows_max,
                width);
    // laid out for the largest round (a caller sizing it by r4r_tower_span_ws_bytes(group, ...) holds at least that);
    // a smaller last round lays the conv's workspace out for its own rows inside the same part
    const TowerWs use = tower_ws(rows_max, width, E, F, V);
    const int64_t tail = n % G;
    const size_t tail_conv = tail ? r4r_textcnn_ws_bytes(tail * per, width, E, F, V) : 0;
    const size_t want = use.total() - use.conv + (tail_conv > use.conv ? tail_conv : use.conv);
    if (ws_bytes < want) {
        set_error("r4r_tower_span_fwd: workspace %zu < %zu bytes (r4r_tower_span_ws_bytes)", ws_bytes, want);
        return R4R_ERR_WORKSPACE;
    }
    const size_t conv_bytes = ws_bytes - (use.total() - use.conv);
    char *base = static_cast<char *>(ws);
    int64_t *docs = reinterpret_cast<int64_t *>(base);
    float *pooled = reinterpret_cast<float *>(base + use.docs);
    int32_t *argmax = reinterpret_cast<int32_t *>(base + use.docs + use.pooled);
    void *conv_ws = base + use.docs + use.pooled + use.argmax;
    // ---- round g: owners [g group, min(n, (g + 1) group)); the ONE stream orders the workspace's reuse
    for (int64_t g = 0, at = 0; at < n; ++g, at += G) {
        const int64_t m = n - at < G ? n - at : G, rows = m * per;
        if (int rc = r4r_tower_build(tok, rev_off, first, nb, owners, ids + at, m, T, R, W, pad, docs,
                                     R > 0 ? neigh + at * NEIGHBOURS : nullptr, stream))
            return rc;
        if (int rc = r4r_textcnn_fwd(table, V, docs, conv_w, conv_b, pooled, argmax, conv_ws, conv_bytes, rows, width, E, F,
                                     stream))
            return rc;
        if (int rc = r4r_linear_fwd(pooled, fc_w, fc_b, latent + at * per * (int64_t)L, rows, F, L, 0, stream)) return rc;
        if (groups_done) *groups_done = g + 1;
    }
    return R4R_OK;
}

// The phrase span (include/r4r.h, "Phrase explanations"): r4r_tower_span_fwd's rounds with r4r_textcnn_phrases in the
// place of r4r_linear_fwd -- the round's pooled / argmax / documents are listed before the next round overwrites them.
extern "C" int r4r_tower_span_phrases(const int32_t *tok, const int64_t *rev_off, const int64_t *first,
                                      const int64_t *nb, int64_t owners, const int64_t *ids, int64_t n, int64_t group,
                                      int T, int R, int W, int64_t pad, const float *table, int64_t V,
                                      const float *conv_w, const float *conv_b, int E, int F, const float *wt,
                                      int64_t wt_stride, int K, int32_t *top_pos, float *top_score,
                                      int32_t *top_filters, int64_t *top_tok, int32_t *n_windows, int64_t *neigh,
                                      void *ws, size_t ws_bytes, int64_t *groups_done, void *stream) {
    if (groups_done) *groups_done = 0;
    if (n == 0) return R4R_OK;
    // ---- everything that can be refused, before the first launch
    R4R_REQUIRE(tok && rev_off && first && ids && table && conv_w && conv_b && ws && (R <= 0 || neigh),
                "r4r_tower_span_phrases: null pointer");
    R4R_REQUIRE(group >= 1, "r4r_tower_span_phrases: group = %lld owners per round, at least 1", (long long)group);
    if (int rc = check_build_shape("r4r_tower_span_phrases", owners, n, T, R, W)) return rc;
    R4R_REQUIRE(E > 0 && E % 4 == 0, "r4r_tower_span_phrases: word_embed_size %d must be a positive multiple of 4 (pad "
                                     "the frozen table and the conv weight on the host otherwise)", E);
    R4R_REQUIRE(F > 0 && F <= 112, "r4r_tower_span_phrases: %d filters > 112 supported", F);
    R4R_REQUIRE(V > 0, "r4r_tower_span_phrases: bad size V=%lld", (long long)V);
    R4R_REQUIRE(K >= 1 && K <= F, "r4r_tower_span_phrases: K=%d outside 1..F=%d", K, F);
    R4R_REQUIRE(wt_stride == 0 || wt_stride == F, "r4r_tower_span_phrases: wt_stride=%lld is neither 0 nor F=%d",
                (long long)wt_stride, F);
    const int per = R > 0 ? R : 1, width = R > 0 ? W : T;
    R4R_REQUIRE(n * per < (1ll << 31), "r4r_tower_span_phrases: %lld rows, 2^31 and more", (long long)(n * per));
    const int64_t G = group < n ? group : n;                // owners of the largest round
    const int64_t rows_max = G * per;
    R4R_REQUIRE(rows_max * (int64_t)((width + 2 + 127) / 128) < (1ll << 31),
                "r4r_tower_span_phrases: %lld rows of %d words per round: the conv's grid is too large",
                (long long)rows_max, width);
    // r4r_tower_span_fwd's layout: the largest round's, the conv's part sized for a smaller last round too
    const TowerWs use = tower_ws(rows_max, width, E, F, V);
    const int64_t tail = n % G;
    const size_t tail_conv = tail ? r4r_textcnn_ws_bytes(tail * per, width, E, F, V) : 0;
    const size_t want = use.total() - use.conv + (tail_conv > use.conv ? tail_conv : use.conv);
    if (ws_bytes < want) {
        set_error("r4r_tower_span_phrases: workspace %zu < %zu bytes (r4r_tower_span_ws_bytes)", ws_bytes, want);
        return R4R_ERR_WORKSPACE;
    }
    const size_t conv_bytes = ws_bytes - (use.total() - use.conv);
    char *base = static_cast<char *>(ws);
    int64_t *docs = reinterpret_cast<int64_t *>(base);
    float *pooled = reinterpret_cast<float *>(base + use.docs);
    int32_t *argmax = reinterpret_cast<int32_t *>(base + use.docs + use.pooled);
    void *conv_ws = base + use.docs + use.pooled + use.argmax;
    // ---- round g: owners [g group, min(n, (g + 1) group)); the ONE stream orders the workspace's reuse
    for (int64_t g = 0, at = 0; at < n; ++g, at += G) {
        const int64_t m = n - at < G ? n - at : G, rows = m * per, row0 = at * per;
        if (int rc = r4r_tower_build(tok, rev_off, first, nb, owners, ids + at, m, T, R, W, pad, docs,
                                     R > 0 ? neigh + at * NEIGHBOURS : nullptr, stream))
            return rc;
        if (int rc = r4r_textcnn_fwd(table, V, docs, conv_w, conv_b, pooled, argmax, conv_ws, conv_bytes, rows, width, E, F,
                                     stream))
            return rc;
        if (int rc = r4r_textcnn_phrases(pooled, argmax, wt && wt_stride ? wt + row0 * wt_stride : wt, wt_stride, docs, rows,
                                         width, F, K, top_pos ? top_pos + row0 * K : nullptr,
                                         top_score ? top_score + row0 * K : nullptr,
                                         top_filters ? top_filters + row0 * K : nullptr,
                                         top_tok ? top_tok + row0 * K * 3 : nullptr,
                                         n_windows ? n_windows + row0 : nullptr, stream))
            return rc;
        if (groups_done) *groups_done = g + 1;
    }
    return R4R_OK;
}

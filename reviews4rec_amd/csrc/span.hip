// K training steps per host call (include/r4r.h, "spans"): the loop body of main.py:23-60 --
//     for data, y in reader.iter(): zero_grad, forward, loss, backward, optimizer.step()
// -- enqueued from C for K consecutive FULL batches of an epoch: the loader's batch construction
// (r4r_batch_build) for a GROUP of batches per launch, then the family's native step per batch with
// its per-step values (batch pointers, Adam step, dropout stream position, token buffer, sweep
// schedule) advanced here exactly as reviews4rec_amd/engine.py advances them between two
// train_step calls.  Host code only: every kernel is the one the per-step entry points launch, so
// a span and K single steps give identical bits (tests/test_gpu_span.py).  The forward-only counterpart -- the
// scoring spans of a validation / ranking pass -- is at the end of the file.
//
// Why groups: one r4r_batch_build is a chain of four dependent loads (rating -> owner -> review
// offsets -> tokens), ~6 us whatever it builds; G batches per launch cost little more than one,
// and the next group is enqueued before the last step of the current one, so no step waits for it
// beyond its share.  The ring holds two groups; a group's slot is last read by the final step of
// the group before the previous one's successor -- everything is ordered by the ONE stream.
#include "common.h"

namespace r4r {

constexpr int NB = 10;                                      // neighbour ids per side (data.py:273-279)

struct SpanLoader {
    const int32_t *user_tok, *item_tok, *held_tok;
    const int64_t *user_rev_off, *user_first, *user_nb, *item_rev_off, *item_first, *item_nb, *held_off;
    const int64_t *u, *i, *ku, *ki, *held;
    const float *y;
    int train, T, R, W;
    int64_t pad_user, pad_item;
    int64_t *ring;
    int64_t stride, N, G, B;
    const uint64_t *resident;                               // HOST table [G][8] of built batches, cycled (word 27)
    bool review;                                            // false: ids only (iter_simple, data.py:336-372)
    int64_t doc() const { return R > 0 ? (int64_t)R * W : T; }
    int64_t full_batches() const { return B > 0 ? N / B : 0; }
    int64_t group_ratings(int64_t g) const {                // ratings of the full batches in group g
        const int64_t left = full_batches() * B - g * G * B;
        return left < G * B ? left : G * B;
    }
};

struct SpanBatch {                                          // device pointers of one batch (the 7-slot list + y)
    const int64_t *this_doc, *who, *what, *user_doc, *item_doc, *uid, *iid;
    const float *y;
};

// scoring: a forward-only pass (the scoring spans below) -- word 15 may be 0, there is nothing to train on.
static int decode_loader(const uint64_t *w, SpanLoader &L, bool scoring = false) {
    R4R_REQUIRE(w, "span: null loader descriptor");
    auto p32 = [&](int k) { return reinterpret_cast<const int32_t *>(w[k]); };
    auto p64 = [&](int k) { return reinterpret_cast<const int64_t *>(w[k]); };
    L.user_tok = p32(0); L.user_rev_off = p64(1); L.user_first = p64(2); L.user_nb = p64(3);
    L.item_tok = p32(4); L.item_rev_off = p64(5); L.item_first = p64(6); L.item_nb = p64(7);
    L.held_tok = p32(8); L.held_off = p64(9);
    L.u = p64(10); L.i = p64(11); L.ku = p64(12); L.ki = p64(13); L.held = p64(14);
    L.y = reinterpret_cast<const float *>(w[15]);
    L.train = (int)w[16]; L.T = (int)w[17]; L.R = (int)w[18]; L.W = (int)w[19];
    L.pad_user = (int64_t)w[20]; L.pad_item = (int64_t)w[21];
    L.ring = reinterpret_cast<int64_t *>(w[22]);
    L.stride = (int64_t)w[23]; L.N = (int64_t)w[24]; L.G = (int64_t)w[25]; L.B = (int64_t)w[26];
    L.resident = reinterpret_cast<const uint64_t *>(w[27]);
    L.review = L.ring != nullptr;
    if (L.resident) {
        R4R_REQUIRE(!L.ring && L.G > 0 && L.B > 0 && L.N >= 0, "span: a resident descriptor has a table of G > 0 batches and no ring");
        return R4R_OK;
    }
    R4R_REQUIRE(L.u && L.i && (L.y || scoring) && L.N >= 0 && L.B > 0, "span: the descriptor needs u, i, y and a batch size");
    if (L.review) {
        R4R_REQUIRE(L.G > 0 && L.stride >= L.G * L.B * (3 * L.doc() + 2 * NB),
                    "span: ring stride %lld < a group of %lld x %lld ratings", (long long)L.stride, (long long)L.G,
                    (long long)L.B);
        R4R_REQUIRE(L.ku && L.ki && L.held, "span: a review loader needs ku, ki, held");
    }
    return R4R_OK;
}

// nb_item: r4r_batch_build's (the negatives' rows report the POSITIVE item's reviewers, data.py:398); null: i.
static int build_group(const SpanLoader &L, int64_t g, hipStream_t st, const int64_t *nb_item = nullptr) {
    const int64_t at = g * L.G * L.B, n = L.group_ratings(g);
    return r4r_batch_build(L.user_tok, L.user_rev_off, L.user_first, L.user_nb, L.item_tok, L.item_rev_off,
                           L.item_first, L.item_nb, L.held_tok, L.held_off, L.u + at, L.i + at, (nb_item ? nb_item : L.i) + at, L.ku + at,
                           L.ki + at, L.held + at, L.train, L.ring + (g & 1) * L.stride, n, L.T, L.R, L.W, L.pad_user,
                           L.pad_item, st);
}

static SpanBatch batch_at(const SpanLoader &L, int64_t b) {
    SpanBatch s{};
    if (L.resident) {
        const uint64_t *t = L.resident + (b % L.G) * 8;
        auto p64 = [&](int k) { return reinterpret_cast<const int64_t *>(t[k]); };
        s.this_doc = p64(0); s.who = p64(1); s.what = p64(2); s.user_doc = p64(3); s.item_doc = p64(4);
        s.uid = p64(5); s.iid = p64(6); s.y = reinterpret_cast<const float *>(t[7]);
        return s;
    }
    s.uid = L.u + b * L.B; s.iid = L.i + b * L.B; s.y = L.y ? L.y + b * L.B : nullptr;
    if (!L.review) return s;
    const int64_t g = b / L.G, j = b - g * L.G, n = L.group_ratings(g), doc = L.doc();
    const int64_t *base = L.ring + (g & 1) * L.stride;
    s.this_doc = base + j * L.B * doc;
    s.who = base + n * doc + j * L.B * NB;
    s.what = base + n * doc + n * NB + j * L.B * NB;
    s.user_doc = base + n * doc + 2 * n * NB + j * L.B * doc;
    s.item_doc = base + 2 * n * doc + 2 * n * NB + j * L.B * doc;
    return s;
}

// step(k, batch, next batch or nullptr) -> rc.  `announce`: a full batch follows the span and the caller wants it
// announced to the last step (its token marks ride on that step's backward launch).
template <class Step>
static int run_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce, int64_t *built_group,
                    int64_t *steps_done, hipStream_t st, Step step) {
    SpanLoader L;
    if (int rc = decode_loader(loader, L)) return rc;
    R4R_REQUIRE(first_batch >= 0 && steps >= 0 && first_batch + steps + (announce ? 1 : 0) <= L.full_batches(),
                "span: batches %lld .. %lld (+%d announced) of %lld full ones", (long long)first_batch,
                (long long)(first_batch + steps), announce ? 1 : 0, (long long)L.full_batches());
    if (steps_done) *steps_done = 0;
    R4R_REQUIRE(!L.review || built_group, "span: built_group is the ring's state, it cannot be null");
    auto need = [&](int64_t b) -> int {
        if (!L.review) return R4R_OK;
        const int64_t g = b / L.G;
        if (*built_group >= g) return R4R_OK;
        // (a span never skips a group: the slot of g was last read by a step before the one being enqueued)
        if (int rc = build_group(L, g, st)) return rc;
        *built_group = g;
        return R4R_OK;
    };
    for (int64_t k = 0; k < steps; ++k) {
        const int64_t b = first_batch + k;
        const bool has_next = k + 1 < steps || announce;
        if (int rc = need(b)) return rc;
        if (has_next)
            if (int rc = need(b + 1)) return rc;
        const SpanBatch cur = batch_at(L, b), nxt = has_next ? batch_at(L, b + 1) : SpanBatch{};
        if (int rc = step(k, cur, has_next ? &nxt : nullptr)) return rc;
        if (steps_done) *steps_done = k + 1;
    }
    return R4R_OK;
}

// The documents a family's step will read (R = 0: one T-token document per rating; R > 0: NARRE's R x T reviews and
// NB neighbour ids per side) against those the descriptor's ring holds -- checked before anything is enqueued: the
// step indexes the ring's blocks by ITS shape, so a mismatch reads tokens as ids and writes row tags out of bounds.
// A resident table (word 27) carries no shape; NARRE's step still reads b*R + r of its NB-wide neighbour lists.
static int check_doc_shape(const uint64_t *loader, const char *who, int R, int T, int64_t *steps_done,
                           bool scoring = false) {
    if (steps_done) *steps_done = 0;
    SpanLoader L;
    if (int rc = decode_loader(loader, L, scoring)) return rc;
    R4R_REQUIRE(R == 0 || R == NB, "%s: R = %d reviews, but the loader holds %d neighbour ids per rating", who, R, NB);
    if (L.resident) return R4R_OK;
    R4R_REQUIRE(L.review, "%s: the descriptor is an ids-only loader, the step reads documents", who);
    if (R == 0)
        R4R_REQUIRE(L.R == 0 && L.T == T, "%s: T = %d, the descriptor builds documents of %s %d", who, T,
                    L.R ? "R x W =" : "T =", L.R ? L.R * L.W : L.T);
    else
        R4R_REQUIRE(L.R == R && L.W == T, "%s: R x T = %d x %d, the descriptor builds %d x %d reviews", who, R, T, L.R,
                    L.W);
    return R4R_OK;
}

struct Sweep {                                              // engine.py _SweepSchedule, one step at a time
    int period, want;
    int64_t base;
    int all() const { return (want != period || period == 1) ? 1 : 0; }
    void done(int64_t step) { if (all()) { base = step; period = want; } }
};

}  // namespace r4r

using namespace r4r;

extern "C" int r4r_span_build(const uint64_t *loader, int64_t batch, int64_t *built_group, void *stream) {
    SpanLoader L;
    if (int rc = decode_loader(loader, L)) return rc;
    R4R_REQUIRE(L.review && built_group && batch >= 0 && batch < L.full_batches(), "span_build: bad batch %lld",
                (long long)batch);
    const int64_t g = batch / L.G;
    if (*built_group >= g) return R4R_OK;
    if (int rc = build_group(L, g, as_stream(stream))) return rc;
    *built_group = g;
    return R4R_OK;
}

extern "C" int r4r_span_batch(const uint64_t *loader, int64_t batch, uint64_t *slots) {
    SpanLoader L;
    if (int rc = decode_loader(loader, L)) return rc;
    R4R_REQUIRE(slots && batch >= 0 && batch < L.full_batches(), "span_batch: bad batch %lld", (long long)batch);
    const SpanBatch s = batch_at(L, batch);
    const void *p[8] = {s.this_doc, s.who, s.what, s.user_doc, s.item_doc, s.uid, s.iid, s.y};
    for (int k = 0; k < 8; ++k) slots[k] = reinterpret_cast<uint64_t>(p[k]);
    return R4R_OK;
}

extern "C" int r4r_deepconn_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                                 int64_t *built_group, int64_t *steps_done, const float *table, int64_t V, float *flat_p, float *flat_g,
                                 float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes, int T, int E,
                                 int L, float dropout_p, int training, uint64_t seed, uint64_t offset, uint64_t draws_per_step,
                                 float inv_denom, int conv_algo, int token_buffer, int tokens_ready, float *flat_m, float *flat_v,
                                 float lr, double beta1, double beta2, float eps, float weight_decay,
                                 int64_t adam_step, void *stream) {
    R4R_REQUIRE(flat_g && flat_m && flat_v && adam_step >= 1, "deepconn_span: training steps only (gradients, moments, adam_step >= 1)");
    if (int rc = check_doc_shape(loader, "deepconn_span", 0, T, steps_done)) return rc;
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    return run_span(loader, first_batch, steps, announce, built_group, steps_done, as_stream(stream),
                    [&](int64_t k, const SpanBatch &c, const SpanBatch *n) {
                        return r4r_deepconn_step(table, V, c.user_doc, c.item_doc, c.y, flat_p, flat_g, pred, se,
                                                 sse_accum, ws, ws_bytes, B, T, E, L, dropout_p, training, seed,
                                                 offset + (uint64_t)k * draws_per_step, inv_denom, conv_algo,
                                                 (token_buffer + (int)k) & 1, k ? 1 : tokens_ready,
                                                 n ? n->user_doc : nullptr, n ? n->item_doc : nullptr, flat_m, flat_v,
                                                 lr, beta1, beta2, eps, weight_decay, adam_step + k, stream);
                    });
}

// ---- data parallel: the headline family's span with the gradient exchange between every step's
// gradients and its update, all of it enqueued from C.  The collective is RCCL's own entry point, called through the
// address the caller resolved in the library it already holds (reviews4rec_amd/dist.py: StreamRccl) on the
// communicator it built -- no second copy of RCCL in the process, nothing linked here.
typedef int (*rccl_allreduce_fn)(const void *, void *, size_t, int, int, void *, void *);
typedef int (*rccl_allgather_fn)(const void *, void *, size_t, int, void *, void *);
constexpr int RCCL_FLOAT32 = 7, RCCL_SUM = 0;              // ncclDataType_t / ncclRedOp_t (rccl.h)

extern "C" int r4r_deepconn_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                                    int64_t *built_group, int64_t *steps_done, const float *table, int64_t V,
                                    float *flat_p, float *flat_g, float *pred, float *se, float *sse_accum, void *ws,
                                    size_t ws_bytes, int T, int E, int L, float dropout_p, int training, uint64_t seed,
                                    uint64_t offset, uint64_t draws_per_step, float inv_denom, int conv_algo,
                                    int token_buffer, int tokens_ready, float *flat_m, float *flat_v, int64_t total,
                                    float lr, double beta1, double beta2, float eps, float weight_decay,
                                    int64_t adam_step, int exchange, void *collective, void *comm, int world,
                                    float *gathered, void *stream) {
    R4R_REQUIRE(flat_g && flat_m && flat_v && adam_step >= 1 && total > 0, "deepconn_span_dp: training steps only");
    R4R_REQUIRE(collective && comm && world >= 1 && (exchange == 0 || (exchange == 1 && gathered)),
                "deepconn_span_dp: exchange 0 (all-reduce) or 1 (all-gather into `gathered` [world][total]) with RCCL's "
                "entry point and a communicator");
    if (int rc = check_doc_shape(loader, "deepconn_span_dp", 0, T, steps_done)) return rc;
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    return run_span(
        loader, first_batch, steps, announce, built_group, steps_done, as_stream(stream),
        [&](int64_t k, const SpanBatch &c, const SpanBatch *n) {
            if (int rc = r4r_deepconn_step(table, V, c.user_doc, c.item_doc, c.y, flat_p, flat_g, pred, se, sse_accum, ws,
                                           ws_bytes, B, T, E, L, dropout_p, training, seed,
                                           offset + (uint64_t)k * draws_per_step, inv_denom, conv_algo,
                                           (token_buffer + (int)k) & 1, k ? 1 : tokens_ready, n ? n->user_doc : nullptr,
                                           n ? n->item_doc : nullptr, nullptr, nullptr, lr, beta1, beta2, eps,
                                           weight_decay, 0, stream))
                return rc;
            if (exchange == 0) {
                const int rc = reinterpret_cast<rccl_allreduce_fn>(collective)(flat_g, flat_g, (size_t)total, RCCL_FLOAT32,
                                                                              RCCL_SUM, comm, stream);
                if (rc) { set_error("deepconn_span_dp: ncclAllReduce returned %d", rc); return R4R_ERR_LAUNCH; }
                const uint64_t p1[1] = {(uint64_t)flat_p}, g1[1] = {(uint64_t)flat_g}, m1[1] = {(uint64_t)flat_m},
                               v1[1] = {(uint64_t)flat_v};
                const int64_t n1[1] = {total};
                return r4r_adam_multi(1, p1, g1, m1, v1, n1, lr, beta1, beta2, eps, weight_decay, adam_step + k, nullptr,
                                      stream);
            }
            const int rc = reinterpret_cast<rccl_allgather_fn>(collective)(flat_g, gathered, (size_t)total, RCCL_FLOAT32,
                                                                          comm, stream);
            if (rc) { set_error("deepconn_span_dp: ncclAllGather returned %d", rc); return R4R_ERR_LAUNCH; }
            return r4r_adam_gathered(flat_p, gathered, world, flat_g, flat_m, flat_v, total, lr, beta1, beta2, eps,
                                     weight_decay, adam_step + k, stream);
        });
}

extern "C" int r4r_deepconnpp_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                                   int64_t *built_group, int64_t *steps_done, const float *table, int64_t V, float *flat_p, float *flat_g,
                                   float *flat_m, float *flat_v, const uint64_t *rows_p, const uint64_t *rows_m,
                                   const uint64_t *rows_v, int64_t n_users, int64_t n_items, float *pred, float *se,
                                   float *sse_accum, void *ws, size_t ws_bytes, int T, int E, int L, float dropout_p,
                                   int training, uint64_t seed, uint64_t offset, uint64_t draws_per_step, float inv_denom,
                                   int conv_algo, int token_buffer, int tokens_ready, float lr, double beta1, double beta2, float eps,
                                   float weight_decay, int64_t adam_step, void *stream) {
    R4R_REQUIRE(flat_g && flat_m && flat_v && adam_step >= 1, "deepconnpp_span: training steps only");
    if (int rc = check_doc_shape(loader, "deepconnpp_span", 0, T, steps_done)) return rc;
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    return run_span(loader, first_batch, steps, announce, built_group, steps_done, as_stream(stream),
                    [&](int64_t k, const SpanBatch &c, const SpanBatch *n) {
                        return r4r_deepconnpp_step(table, V, c.user_doc, c.item_doc, c.uid, c.iid, c.y, flat_p, flat_g,
                                                   flat_m, flat_v, rows_p, rows_m, rows_v, n_users, n_items, pred, se,
                                                   sse_accum, ws, ws_bytes, B, T, E, L, dropout_p, training, seed,
                                                   offset + (uint64_t)k * draws_per_step, inv_denom, conv_algo,
                                                   (token_buffer + (int)k) & 1, k ? 1 : tokens_ready,
                                                   n ? n->user_doc : nullptr, n ? n->item_doc : nullptr, lr, beta1,
                                                   beta2, eps, weight_decay, adam_step + k, stream);
                    });
}

extern "C" int r4r_narre_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                              int64_t *built_group, int64_t *steps_done, const float *table, int64_t V, float *flat_p, float *flat_g,
                              float *flat_m, float *flat_v, const uint64_t *rows_p, const uint64_t *rows_m,
                              const uint64_t *rows_v, int64_t n_users, int64_t n_items, float *pred, float *se,
                              float *sse_accum, void *ws, size_t ws_bytes, int R, int T, int E, int L,
                              float dropout_p, int training, uint64_t seed, uint64_t offset, uint64_t draws_per_step,
                              float inv_denom, int conv_algo, int token_buffer, int tokens_ready, float lr, double beta1, double beta2,
                              float eps, float weight_decay, int64_t adam_step, void *stream) {
    R4R_REQUIRE(flat_g && flat_m && flat_v && adam_step >= 1, "narre_span: training steps only");
    if (int rc = check_doc_shape(loader, "narre_span", R, T, steps_done)) return rc;
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    return run_span(loader, first_batch, steps, announce, built_group, steps_done, as_stream(stream),
                    [&](int64_t k, const SpanBatch &c, const SpanBatch *n) {
                        // NARRE.py:87-96: reviewed_items = data[2], users_who_reviewed = data[1]
                        return r4r_narre_step(table, V, c.user_doc, c.item_doc, c.what, c.who, c.uid, c.iid, c.y,
                                              flat_p, flat_g, flat_m, flat_v, rows_p, rows_m, rows_v, n_users, n_items,
                                              pred, se, sse_accum, ws, ws_bytes, B, R, T, E, L, dropout_p, training,
                                              seed, offset + (uint64_t)k * draws_per_step, inv_denom, conv_algo,
                                              (token_buffer + (int)k) & 1, k ? 1 : tokens_ready,
                                              n ? n->user_doc : nullptr, n ? n->item_doc : nullptr, lr, beta1, beta2,
                                              eps, weight_decay, adam_step + k, stream);
                    });
}

extern "C" int r4r_transnet_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                                 int64_t *built_group, int64_t *steps_done, const float *table, int64_t V, float *flat_p, float *flat_g,
                                 float *flat_m, float *flat_v, const uint64_t *rows_p, const uint64_t *rows_m,
                                 const uint64_t *rows_v, int64_t n_users, int64_t n_items, float *pred, float *se,
                                 float *sse_accum, void *ws, size_t ws_bytes, int T, int E, int L, int plus,
                                 float dropout_p, int training, uint64_t seed, uint64_t offset, uint64_t draws_per_step,
                                 float inv_denom, int conv_algo, int token_buffer, int tokens_ready, int sweep_period,
                                 int sweep_want, int64_t *sweep_base, int *sweep_period_out, float lr, double beta1,
                                 double beta2, float eps, float weight_decay, int64_t adam_step, void *stream) {
    R4R_REQUIRE(flat_g && flat_m && flat_v && adam_step >= 1 && sweep_base && sweep_period_out,
                "transnet_span: training steps only; sweep_base / sweep_period_out are the schedule's state");
    if (int rc = check_doc_shape(loader, "transnet_span", 0, T, steps_done)) {
        *sweep_period_out = sweep_period;                   // (nothing was enqueued: the schedule is the one passed in)
        return rc;
    }
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    Sweep sw{sweep_period, sweep_want, *sweep_base};
    const int rc = run_span(
        loader, first_batch, steps, announce, built_group, steps_done, as_stream(stream),
        [&](int64_t k, const SpanBatch &c, const SpanBatch *n) {
            const int rc1 = r4r_transnet_step(
                table, V, c.user_doc, c.item_doc, c.this_doc, c.uid, c.iid, c.y, flat_p, flat_g, flat_m, flat_v, rows_p,
                rows_m, rows_v, n_users, n_items, pred, se, sse_accum, ws, ws_bytes, B, T, E, L, plus, dropout_p,
                training, seed, offset + (uint64_t)k * draws_per_step, inv_denom, conv_algo, (token_buffer + (int)k) & 1,
                k ? 1 : tokens_ready, n ? n->user_doc : nullptr, n ? n->item_doc : nullptr, n ? n->this_doc : nullptr,
                sw.period, sw.base, sw.all(), lr, beta1, beta2, eps, weight_decay, adam_step + k, stream);
            if (rc1 == R4R_OK) sw.done(adam_step + k);
            return rc1;
        });
    *sweep_base = sw.base;
    *sweep_period_out = sw.period;
    return rc;
}

extern "C" int r4r_mf_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int64_t *steps_done, const uint64_t *p,
                           const uint64_t *m, const uint64_t *v, int64_t n_users, int64_t n_items, int D, float *pred,
                           float *se, float *sse_accum, void *ws, size_t ws_bytes, float dropout_p, int training,
                           uint64_t seed, uint64_t offset, uint64_t draws_per_step, float inv_denom, int sweep_period, int sweep_want,
                           int64_t *sweep_base, int *sweep_period_out, float lr, double beta1, double beta2, float eps,
                           float weight_decay, int64_t adam_step, void *stream) {
    R4R_REQUIRE(m && v && adam_step >= 1 && sweep_base && sweep_period_out, "mf_span: training steps only");
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    Sweep sw{sweep_period, sweep_want, *sweep_base};
    const int rc = run_span(loader, first_batch, steps, 0, nullptr, steps_done, as_stream(stream),
                            [&](int64_t k, const SpanBatch &c, const SpanBatch *) {
                                const int rc1 = r4r_mf_step(c.uid, c.iid, c.y, p, m, v, n_users, n_items, D, pred, se,
                                                            sse_accum, ws, ws_bytes, B, dropout_p, training, seed,
                                                            offset + (uint64_t)k * draws_per_step, inv_denom, sw.period, sw.base,
                                                            sw.all(), lr, beta1, beta2, eps, weight_decay,
                                                            adam_step + k, stream);
                                if (rc1 == R4R_OK) sw.done(adam_step + k);
                                return rc1;
                            });
    *sweep_base = sw.base;
    *sweep_period_out = sw.period;
    return rc;
}

extern "C" int r4r_idnet_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int64_t *steps_done, int variant, float *flat_p,
                              float *flat_g, float *flat_m, float *flat_v, const uint64_t *rows_p,
                              const uint64_t *rows_m, const uint64_t *rows_v, int64_t n_users, int64_t n_items,
                              float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes, int L,
                              float dropout_p, int training, uint64_t seed, uint64_t offset, uint64_t draws_per_step,
                              float inv_denom, int sweep_period, int sweep_want, int64_t *sweep_base,
                              int *sweep_period_out, float lr, double beta1, double beta2, float eps,
                              float weight_decay, int64_t adam_step, void *stream) {
    R4R_REQUIRE(flat_g && flat_m && flat_v && adam_step >= 1 && sweep_base && sweep_period_out,
                "idnet_span: training steps only");
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    Sweep sw{sweep_period, sweep_want, *sweep_base};
    const int rc = run_span(loader, first_batch, steps, 0, nullptr, steps_done, as_stream(stream),
                            [&](int64_t k, const SpanBatch &c, const SpanBatch *) {
                                const int rc1 = r4r_idnet_step(variant, c.uid, c.iid, c.y, flat_p, flat_g, flat_m, flat_v,
                                                               rows_p, rows_m, rows_v, n_users, n_items, pred, se,
                                                               sse_accum, ws, ws_bytes, B, L, dropout_p, training, seed,
                                                               offset + (uint64_t)k * draws_per_step, inv_denom,
                                                               sw.period, sw.base, sw.all(), lr, beta1, beta2, eps,
                                                               weight_decay, adam_step + k, stream);
                                if (rc1 == R4R_OK) sw.done(adam_step + k);
                                return rc1;
                            });
    *sweep_base = sw.base;
    *sweep_period_out = sw.period;
    return rc;
}

// ---- data parallel for the other native families: each is its family's span with the exchange of the per-step
// data-parallel path (reviews4rec_amd/engine.py: _train_step_dp / _dp_rows) between every step's gradients and its
// updates -- the same launches, arguments, collectives and order, so an epoch through these leaves the bits of the
// per-step loop.  Only the exchange forms each family takes at ordinary sizes are here (the packed blocks); beyond them
// the engine runs the step through train_step.
namespace r4r {

struct DpComm {                                             // RCCL's entry points, resolved by the caller (dist.StreamRccl)
    void *allreduce, *allgather, *comm;
    int world;
    const char *who;
    int reduce(float *g, int64_t n, void *stream) const {   // in place, float32 sum (StreamRccl.all_reduce)
        const int rc = reinterpret_cast<rccl_allreduce_fn>(allreduce)(g, g, (size_t)n, RCCL_FLOAT32, RCCL_SUM, comm, stream);
        if (rc) { set_error("%s: ncclAllReduce returned %d", who, rc); return R4R_ERR_LAUNCH; }
        return R4R_OK;
    }
    int gather(const void *block, void *blocks, size_t bytes, void *stream) const {   // 4-byte words (StreamRccl.all_gather)
        const int rc = reinterpret_cast<rccl_allgather_fn>(allgather)(block, blocks, bytes / 4, RCCL_FLOAT32, comm, stream);
        if (rc) { set_error("%s: ncclAllGather returned %d", who, rc); return R4R_ERR_LAUNCH; }
        return R4R_OK;
    }
};

// The dense half of a step (engine.py _train_step_dp): the all-reduced flat gradient into the flat Adam.
static int dp_dense(const DpComm &c, float *flat_p, float *flat_g, float *flat_m, float *flat_v, int64_t total, float lr,
                    double beta1, double beta2, float eps, float weight_decay, int64_t step, void *stream) {
    if (int rc = c.reduce(flat_g, total, stream)) return rc;
    const uint64_t p1[1] = {(uint64_t)flat_p}, g1[1] = {(uint64_t)flat_g}, m1[1] = {(uint64_t)flat_m}, v1[1] = {(uint64_t)flat_v};
    const int64_t n1[1] = {total};
    return r4r_adam_multi(1, p1, g1, m1, v1, n1, lr, beta1, beta2, eps, weight_decay, step, nullptr, stream);
}

// engine.gather_entry_fields: this rank's entries packed into one block, ONE all-gather, unpacked into `dst`.
static int dp_fields(const DpComm &c, int nf, const uint64_t *src, const int *widths, const int *ones, int64_t n,
                     int64_t B_pad, void *block, void *blocks, const uint64_t *dst, void *stream) {
    const size_t nbytes = r4r_dp_block_bytes(nf, widths, B_pad);
    if (int rc = r4r_dp_pack(nf, src, widths, ones, n, B_pad, block, stream)) return rc;
    if (int rc = c.gather(block, blocks, nbytes > 4 ? nbytes : 4, stream)) return rc;
    return r4r_dp_unpack(nf, dst, widths, blocks, c.world, B_pad, stream);
}

// Checked before anything is enqueued (and with *steps_done = 0 already): the collectives' addresses and communicator.
static int dp_comm_ok(const char *who, bool reduce, void *allreduce, void *allgather, void *comm, int world) {
    R4R_REQUIRE((!reduce || allreduce) && allgather && comm && world >= 1,
                "%s: RCCL's entry points (%s), a communicator and world >= 1", who,
                reduce ? "ncclAllReduce, ncclAllGather" : "ncclAllGather");
    return R4R_OK;
}

}  // namespace r4r

extern "C" int r4r_narre_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                                 int64_t *built_group, int64_t *steps_done, const float *table, int64_t V,
                                 float *flat_p, float *flat_g, float *flat_m, float *flat_v, int64_t total,
                                 const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                                 int64_t n_users, int64_t n_items, float *pred, float *se, float *sse_accum, void *ws,
                                 size_t ws_bytes, int R, int T, int E, int L, float dropout_p, int training,
                                 uint64_t seed, uint64_t offset, uint64_t draws_per_step, float inv_denom,
                                 int conv_algo, int token_buffer, int tokens_ready, float lr, double beta1,
                                 double beta2, float eps, float weight_decay, int64_t adam_step, void *allreduce,
                                 void *allgather, void *comm, int world, int64_t B_pad, void *block, void *blocks,
                                 void *stream) {
    if (steps_done) *steps_done = 0;
    R4R_REQUIRE(flat_g && flat_m && flat_v && rows_m && rows_v && adam_step >= 1 && total > 0,
                "narre_span_dp: training steps only (gradients, moments, adam_step >= 1)");
    if (int rc = dp_comm_ok("narre_span_dp", true, allreduce, allgather, comm, world)) return rc;
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    R4R_REQUIRE(R == NB, "narre_span_dp: R = %d reviews, the ring holds %d neighbour ids per rating", R, NB);
    R4R_REQUIRE(block && blocks && B <= B_pad && (int64_t)world * B_pad * (1 + R) <= 16384 && L <= 32,
                "narre_span_dp: the packed blocks (world x B_pad x (1 + R) <= 16384 entries, L <= 32, B <= B_pad)");
    if (int rc = check_doc_shape(loader, "narre_span_dp", R, T, steps_done)) return rc;
    const DpComm c{allreduce, allgather, comm, world, "narre_span_dp"};
    const size_t nbytes = r4r_narre_dp_block_bytes(B_pad, R, L);
    return run_span(
        loader, first_batch, steps, announce, built_group, steps_done, as_stream(stream),
        [&](int64_t k, const SpanBatch &b, const SpanBatch *n) {
            const int64_t step = adam_step + k;
            // NARRE.py:87-96: reviewed_items = data[2], users_who_reviewed = data[1]; gradients only
            if (int rc = r4r_narre_step(table, V, b.user_doc, b.item_doc, b.what, b.who, b.uid, b.iid, b.y, flat_p,
                                        flat_g, nullptr, nullptr, rows_p, nullptr, nullptr, n_users, n_items, pred, se,
                                        sse_accum, ws, ws_bytes, B, R, T, E, L, dropout_p, training, seed,
                                        offset + (uint64_t)k * draws_per_step, inv_denom, conv_algo,
                                        (token_buffer + (int)k) & 1, k ? 1 : tokens_ready, n ? n->user_doc : nullptr,
                                        n ? n->item_doc : nullptr, lr, beta1, beta2, eps, weight_decay, step, stream))
                return rc;
            if (int rc = dp_dense(c, flat_p, flat_g, flat_m, flat_v, total, lr, beta1, beta2, eps, weight_decay, step,
                                  stream))
                return rc;
            if (int rc = r4r_narre_dp_block(ws, ws_bytes, B, R, T, E, L, V, n_users, n_items, block, B_pad, stream))
                return rc;
            if (int rc = c.gather(block, blocks, nbytes, stream)) return rc;
            return r4r_narre_rows_apply_blocks(blocks, world, B_pad, rows_p, rows_m, rows_v, n_users, n_items, ws,
                                               ws_bytes, B, R, T, E, L, V, lr, beta1, beta2, eps, weight_decay, step,
                                               stream);
        });
}

extern "C" int r4r_deepconnpp_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                                      int64_t *built_group, int64_t *steps_done, const float *table, int64_t V,
                                      float *flat_p, float *flat_g, float *flat_m, float *flat_v, int64_t total,
                                      const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                                      int64_t n_users, int64_t n_items, float *pred, float *se, float *sse_accum,
                                      void *ws, size_t ws_bytes, int T, int E, int L, float dropout_p, int training,
                                      uint64_t seed, uint64_t offset, uint64_t draws_per_step, float inv_denom,
                                      int conv_algo, int token_buffer, int tokens_ready, float lr, double beta1,
                                      double beta2, float eps, float weight_decay, int64_t adam_step, void *allreduce,
                                      void *allgather, void *comm, int world, int64_t B_pad, void *block,
                                      void *blocks, const uint64_t *gathered, void *stream) {
    if (steps_done) *steps_done = 0;
    R4R_REQUIRE(flat_g && flat_m && flat_v && rows_m && rows_v && adam_step >= 1 && total > 0,
                "deepconnpp_span_dp: training steps only (gradients, moments, adam_step >= 1)");
    if (int rc = dp_comm_ok("deepconnpp_span_dp", true, allreduce, allgather, comm, world)) return rc;
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    R4R_REQUIRE(block && blocks && gathered && gathered[0] && gathered[1] && gathered[2] && B <= B_pad &&
                    (int64_t)world * B_pad <= 16384,
                "deepconnpp_span_dp: the exchange buffers (block, blocks, gathered uid / iid / d loss/d pred) and "
                "world x B_pad <= 16384, B <= B_pad");
    if (int rc = check_doc_shape(loader, "deepconnpp_span_dp", 0, T, steps_done)) return rc;
    const DpComm c{allreduce, allgather, comm, world, "deepconnpp_span_dp"};
    const int widths[3] = {2, 2, 1}, ones[3] = {1, 1, 0};   // uid, iid (int64, -1 padding), d loss / d pred
    const uint64_t g = (uint64_t)ws + r4r_deepconnpp_ws_offset(B, T, E, L, V, n_users, n_items, 5);
    return run_span(
        loader, first_batch, steps, announce, built_group, steps_done, as_stream(stream),
        [&](int64_t k, const SpanBatch &b, const SpanBatch *n) {
            const int64_t step = adam_step + k;
            if (int rc = r4r_deepconnpp_step(table, V, b.user_doc, b.item_doc, b.uid, b.iid, b.y, flat_p, flat_g, nullptr,
                                             nullptr, rows_p, nullptr, nullptr, n_users, n_items, pred, se, sse_accum, ws,
                                             ws_bytes, B, T, E, L, dropout_p, training, seed,
                                             offset + (uint64_t)k * draws_per_step, inv_denom, conv_algo,
                                             (token_buffer + (int)k) & 1, k ? 1 : tokens_ready,
                                             n ? n->user_doc : nullptr, n ? n->item_doc : nullptr, lr, beta1, beta2,
                                             eps, weight_decay, step, stream))
                return rc;
            if (int rc = dp_dense(c, flat_p, flat_g, flat_m, flat_v, total, lr, beta1, beta2, eps, weight_decay, step,
                                  stream))
                return rc;
            const uint64_t src[3] = {(uint64_t)b.uid, (uint64_t)b.iid, g};
            if (int rc = dp_fields(c, 3, src, widths, ones, B, B_pad, block, blocks, gathered, stream)) return rc;
            return r4r_deepconnpp_rows_apply(reinterpret_cast<const int64_t *>(gathered[0]),
                                             reinterpret_cast<const int64_t *>(gathered[1]),
                                             reinterpret_cast<const float *>(gathered[2]), world * B_pad, rows_p, rows_m,
                                             rows_v, n_users, n_items, ws, ws_bytes, B, T, E, L, V, lr, beta1, beta2,
                                             eps, weight_decay, step, stream);
        });
}

extern "C" int r4r_transnet_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                                    int64_t *built_group, int64_t *steps_done, const float *table, int64_t V,
                                    float *flat_p, float *flat_g, float *flat_m, float *flat_v, int64_t total,
                                    const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                                    int64_t n_users, int64_t n_items, float *pred, float *se, float *sse_accum,
                                    void *ws, size_t ws_bytes, int T, int E, int L, int plus, float dropout_p,
                                    int training, uint64_t seed, uint64_t offset, uint64_t draws_per_step,
                                    float inv_denom, int conv_algo, int token_buffer, int tokens_ready,
                                    int sweep_period, int sweep_want, int64_t *sweep_base, int *sweep_period_out,
                                    float lr, double beta1, double beta2, float eps, float weight_decay,
                                    int64_t adam_step, void *allreduce, void *allgather, void *comm, int world,
                                    int64_t B_pad, void *block, void *blocks, void *stream) {
    if (steps_done) *steps_done = 0;
    R4R_REQUIRE(flat_g && flat_m && flat_v && adam_step >= 1 && total > 0 && sweep_base && sweep_period_out,
                "transnet_span_dp: training steps only; sweep_base / sweep_period_out are the schedule's state");
    *sweep_period_out = sweep_period;                       // (until a step completes: the schedule passed in)
    if (int rc = dp_comm_ok("transnet_span_dp", true, allreduce, allgather, comm, world)) return rc;
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    R4R_REQUIRE(!plus || (rows_m && rows_v && block && blocks && B <= B_pad && (int64_t)world * B_pad <= 2048),
                "transnet_span_dp: TransNet++ exchanges packed blocks (moments, block, blocks; world x B_pad <= 2048, "
                "B <= B_pad)");
    if (int rc = check_doc_shape(loader, "transnet_span_dp", 0, T, steps_done)) return rc;
    const DpComm c{allreduce, allgather, comm, world, "transnet_span_dp"};
    const size_t nbytes = plus ? r4r_transnet_dp_block_bytes(B_pad) : 0;
    Sweep sw{sweep_period, sweep_want, *sweep_base};
    const int rc = run_span(
        loader, first_batch, steps, announce, built_group, steps_done, as_stream(stream),
        [&](int64_t k, const SpanBatch &b, const SpanBatch *n) {
            const int64_t step = adam_step + k;
            // gradients only; rows_m / rows_v still read, for the catch-up of the rows a rating names
            if (int rc = r4r_transnet_step(
                    table, V, b.user_doc, b.item_doc, b.this_doc, b.uid, b.iid, b.y, flat_p, flat_g, nullptr, nullptr,
                    rows_p, rows_m, rows_v, n_users, n_items, pred, se, sse_accum, ws, ws_bytes, B, T, E, L, plus,
                    dropout_p, training, seed, offset + (uint64_t)k * draws_per_step, inv_denom, conv_algo,
                    (token_buffer + (int)k) & 1, k ? 1 : tokens_ready, n ? n->user_doc : nullptr,
                    n ? n->item_doc : nullptr, n ? n->this_doc : nullptr, sw.period, sw.base, sw.all(), lr, beta1, beta2,
                    eps, weight_decay, step, stream))
                return rc;
            if (int rc = dp_dense(c, flat_p, flat_g, flat_m, flat_v, total, lr, beta1, beta2, eps, weight_decay, step,
                                  stream))
                return rc;
            if (plus) {
                if (int rc = r4r_transnet_dp_block(b.uid, b.iid, ws, ws_bytes, B, T, E, L, V, n_users, n_items, block,
                                                   B_pad, stream))
                    return rc;
                if (int rc = c.gather(block, blocks, nbytes, stream)) return rc;
                if (int rc = r4r_transnet_rows_apply_blocks(blocks, world, B_pad, sw.period, sw.base, sw.all(), rows_p,
                                                            rows_m, rows_v, n_users, n_items, ws, ws_bytes, B, T, E, L,
                                                            V, lr, beta1, beta2, eps, weight_decay, step, stream))
                    return rc;
            }
            sw.done(step);
            return R4R_OK;
        });
    *sweep_base = sw.base;
    *sweep_period_out = sw.period;
    return rc;
}

extern "C" int r4r_idnet_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int64_t *steps_done,
                                 int variant, float *flat_p, float *flat_g, float *flat_m, float *flat_v,
                                 int64_t total, const uint64_t *rows_p, const uint64_t *rows_m,
                                 const uint64_t *rows_v, int64_t n_users, int64_t n_items, float *pred, float *se,
                                 float *sse_accum, void *ws, size_t ws_bytes, int L, float dropout_p, int training,
                                 uint64_t seed, uint64_t offset, uint64_t draws_per_step, float inv_denom,
                                 int sweep_period, int sweep_want, int64_t *sweep_base, int *sweep_period_out,
                                 float lr, double beta1, double beta2, float eps, float weight_decay,
                                 int64_t adam_step, void *allreduce, void *allgather, void *comm, int world,
                                 int64_t B_pad, void *block, void *blocks, const uint64_t *gathered, void *stream) {
    if (steps_done) *steps_done = 0;
    R4R_REQUIRE(flat_g && flat_m && flat_v && rows_m && rows_v && adam_step >= 1 && total > 0 && sweep_base &&
                    sweep_period_out,
                "idnet_span_dp: training steps only; sweep_base / sweep_period_out are the schedule's state");
    *sweep_period_out = sweep_period;
    if (int rc = dp_comm_ok("idnet_span_dp", true, allreduce, allgather, comm, world)) return rc;
    const int ntab = variant == 3 ? 4 : 2, nf = 3 + ntab;  // NeuMF: two table pairs
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    bool have = block && blocks && gathered && variant >= 0 && variant <= 3;
    for (int f = 0; have && f < nf; ++f) have = gathered[f] != 0;
    R4R_REQUIRE(have && B <= B_pad && (int64_t)world * B_pad <= 16384,
                "idnet_span_dp: the exchange buffers (block, blocks, gathered uid / iid / d loss/d pred / %d row "
                "arrays) and world x B_pad <= 16384, B <= B_pad", ntab);
    const DpComm c{allreduce, allgather, comm, world, "idnet_span_dp"};
    int widths[7], ones[7];
    uint64_t src[7];
    for (int f = 0; f < nf; ++f) {                          // uid, iid (int64, -1 padding), d loss / d pred, the rows
        widths[f] = f < 2 ? 2 : (f == 2 ? 1 : L);
        ones[f] = f < 2;
        src[f] = f < 2 ? 0 : (uint64_t)ws + r4r_idnet_ws_offset(variant, B, L, n_users, n_items, f == 2 ? 1 : 4 + f - 3);
    }
    uint64_t gu[2] = {gathered[3], ntab > 2 ? gathered[5] : 0}, gi[2] = {gathered[4], ntab > 2 ? gathered[6] : 0};
    Sweep sw{sweep_period, sweep_want, *sweep_base};
    const int rc = run_span(
        loader, first_batch, steps, 0, nullptr, steps_done, as_stream(stream),
        [&](int64_t k, const SpanBatch &b, const SpanBatch *) {
            const int64_t step = adam_step + k;
            // gradients only; rows_m / rows_v still read, for the catch-up of the rows a rating names
            if (int rc = r4r_idnet_step(variant, b.uid, b.iid, b.y, flat_p, flat_g, nullptr, nullptr, rows_p, rows_m,
                                        rows_v, n_users, n_items, pred, se, sse_accum, ws, ws_bytes, B, L, dropout_p,
                                        training, seed, offset + (uint64_t)k * draws_per_step, inv_denom, sw.period,
                                        sw.base, sw.all(), lr, beta1, beta2, eps, weight_decay, step, stream))
                return rc;
            if (int rc = dp_dense(c, flat_p, flat_g, flat_m, flat_v, total, lr, beta1, beta2, eps, weight_decay, step,
                                  stream))
                return rc;
            src[0] = (uint64_t)b.uid;
            src[1] = (uint64_t)b.iid;
            if (int rc = dp_fields(c, nf, src, widths, ones, B, B_pad, block, blocks, gathered, stream)) return rc;
            if (int rc = r4r_idnet_rows_apply(variant, reinterpret_cast<const int64_t *>(gathered[0]),
                                              reinterpret_cast<const int64_t *>(gathered[1]),
                                              reinterpret_cast<const float *>(gathered[2]), gu, gi, sw.period, sw.base,
                                              sw.all(), world * B_pad, rows_p, rows_m, rows_v, n_users, n_items, ws,
                                              ws_bytes, B, L, lr, beta1, beta2, eps, weight_decay, step, stream))
                return rc;
            sw.done(step);
            return R4R_OK;
        });
    *sweep_base = sw.base;
    *sweep_period_out = sw.period;
    return rc;
}

extern "C" int r4r_mf_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int64_t *steps_done,
                              const uint64_t *p, const uint64_t *m, const uint64_t *v, int64_t n_users,
                              int64_t n_items, int D, float *pred, float *se, float *sse_accum, void *ws,
                              size_t ws_bytes, float dropout_p, int training, uint64_t seed, uint64_t offset,
                              uint64_t draws_per_step, float inv_denom, int sweep_period, int sweep_want,
                              int64_t *sweep_base, int *sweep_period_out, float lr, double beta1, double beta2,
                              float eps, float weight_decay, int64_t adam_step, void *allgather, void *comm, int world,
                              int64_t B_pad, void *block, void *blocks, void *stream) {
    if (steps_done) *steps_done = 0;
    R4R_REQUIRE(m && v && adam_step >= 1 && sweep_base && sweep_period_out,
                "mf_span_dp: training steps only; sweep_base / sweep_period_out are the schedule's state");
    *sweep_period_out = sweep_period;
    if (int rc = dp_comm_ok("mf_span_dp", false, nullptr, allgather, comm, world)) return rc;
    const int64_t B = loader ? (int64_t)loader[26] : 0;
    R4R_REQUIRE(ws && block && blocks && B <= B_pad && (int64_t)world * B_pad <= 16384,
                "mf_span_dp: the exchange buffers (ws, block, blocks) and world x B_pad <= 16384, B <= B_pad");
    const DpComm c{nullptr, allgather, comm, world, "mf_span_dp"};
    const size_t nbytes = r4r_mf_dp_block_bytes(B_pad, D);
    Sweep sw{sweep_period, sweep_want, *sweep_base};
    const int rc = run_span(
        loader, first_batch, steps, 0, nullptr, steps_done, as_stream(stream),
        [&](int64_t k, const SpanBatch &b, const SpanBatch *) {
            const int64_t step = adam_step + k;
            const bool pending = D > 0 && sw.period > 1;   // (rows may carry pending updates: the forward catches them up)
            if (int rc = r4r_mf_grad(b.uid, b.iid, b.y, p, pending ? m : nullptr, pending ? v : nullptr, n_users,
                                     n_items, D, pred, se, block, nullptr, B, B_pad, dropout_p, training, seed,
                                     offset + (uint64_t)k * draws_per_step, inv_denom, pending ? ws : nullptr,
                                     sw.period, sw.base, lr, beta1, beta2, eps, weight_decay, step, stream))
                return rc;
            if (int rc = c.gather(block, blocks, nbytes, stream)) return rc;
            if (int rc = r4r_mf_apply(blocks, world, B_pad, p, m, v, n_users, n_items, D, ws, ws_bytes, sw.period,
                                      sw.base, sw.all(), se, B, sse_accum, lr, beta1, beta2, eps, weight_decay, step,
                                      stream))
                return rc;
            sw.done(step);
            return R4R_OK;
        });
    *sweep_base = sw.base;
    *sweep_period_out = sw.period;
    return rc;
}

// ---------------------------------------------------------------------------------------------------------------------
// Scoring spans (include/r4r.h, "Scoring spans"): the forward-only counterpart -- eval.py:24-40 / 64-78's loop body,
//     for data, y in reader.iter(eval=True) / iter_negs(): output = model(data); criterion(output, y)
// enqueued from C for consecutive FULL launches of n ratings of a split (or of the ranking rows, six candidates per
// row, flattened).  Launch k is the family's own r4r_*_step in the form engine.predict calls it (no gradients, no
// moments, training 0, tokens_ready 0, no next batch), writing pred / se at k * n of split-sized arrays: the kernels
// and their arguments are the per-launch path's, so every score keeps its bits (tests/test_gpu_score_span.py).
// The only kernels of this file are the two small ones below: TransNet's per-rating pair out of the workspace, and
// the HR@1 count over the finished scores.
namespace r4r {

template <class Launch>
static int run_score(const char *who, const uint64_t *loader, const int64_t *nb_item, int64_t first, int64_t launches,
                     int64_t *built_group, int64_t *launches_done, const float *se_out, hipStream_t st, Launch launch) {
    if (launches_done) *launches_done = 0;
    SpanLoader L;
    if (int rc = decode_loader(loader, L, /*scoring=*/true)) return rc;
    R4R_REQUIRE(first >= 0 && launches >= 0 && first + launches <= L.full_batches(),
                "%s: launches %lld .. %lld of %lld full ones", who, (long long)first, (long long)(first + launches),
                (long long)L.full_batches());
    R4R_REQUIRE(!(L.resident && nb_item), "%s: a resident table holds built batches, nb_item has nothing to build", who);
    bool rated = L.y != nullptr;
    if (L.resident)
        for (int64_t j = 0; j < L.G && !rated; ++j) rated = L.resident[j * 8 + 7] != 0;
    R4R_REQUIRE(!rated || se_out, "%s: the descriptor has ratings (y), se_out cannot be null", who);
    R4R_REQUIRE(!L.review || built_group, "%s: built_group is the ring's state, it cannot be null", who);
    auto need = [&](int64_t b) -> int {                     // (as run_span's: groups in order, the next before it is read)
        if (!L.review) return R4R_OK;
        const int64_t g = b / L.G;
        if (*built_group >= g) return R4R_OK;
        if (int rc = build_group(L, g, st, nb_item)) return rc;
        *built_group = g;
        return R4R_OK;
    };
    for (int64_t k = 0; k < launches; ++k) {
        const int64_t b = first + k;
        if (int rc = need(b)) return rc;
        if (k + 1 < launches)
            if (int rc = need(b + 1)) return rc;
        if (int rc = launch(k, batch_at(L, b), L.B)) return rc;
        if (launches_done) *launches_done = k + 1;
    }
    return R4R_OK;
}

// TransNet: columns 1:3 of the workspace's per-rating [n, 3] (target prediction | its SE | transform distance).
__global__ void score_aux_kernel(const float *__restrict__ aux3, float *__restrict__ out2, int64_t n) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) {
        out2[2 * r] = aux3[3 * r + 1];
        out2[2 * r + 1] = aux3[3 * r + 2];
    }
}

// HR@1 (eval.py:79-88) without the scores leaving the device.  One row per lane, 64 rows per wave and pass; a row is
// a HIT when its positive (column 0) is strictly greater than every other column, UNDECIDED when it equals the best of
// the others or the row holds a NaN (torch.topk's tie / NaN order decides those on the host).  Counts are summed per
// wave from the ballots, per workgroup through LDS, then one integer atomic pair: order-independent.
template <int CT>
__global__ void __launch_bounds__(256) rank_top1_kernel(const float *__restrict__ scores, int64_t rows, int C,
                                                         unsigned long long *__restrict__ counts) {
    __shared__ unsigned int part[2][4];
    unsigned int hits = 0, open = 0;                        // wave-uniform
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t passes = (rows + stride - 1) / stride;
    for (int64_t p = 0; p < passes; ++p) {
        const int64_t r = p * stride + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        bool hit = false, und = false;
        if (r < rows) {
            const float *s = scores + r * (CT ? CT : C);
            float pos, best = -INFINITY;
            bool nan = false;
            if (CT == 6) {                                  // the product's shape: three 8-byte loads (24-byte rows)
                const float2 a = reinterpret_cast<const float2 *>(s)[0], b = reinterpret_cast<const float2 *>(s)[1],
                             c = reinterpret_cast<const float2 *>(s)[2];
                pos = a.x;
                const float o[5] = {a.y, b.x, b.y, c.x, c.y};
#pragma unroll
                for (int j = 0; j < 5; ++j) { nan |= o[j] != o[j]; best = fmaxf(best, o[j]); }
            } else {
                pos = s[0];
                for (int j = 1; j < C; ++j) { const float o = s[j]; nan |= o != o; best = fmaxf(best, o); }
            }
            nan |= pos != pos;
            hit = !nan && pos > best;
            und = nan || pos == best;
        }
        hits += (unsigned int)__popcll(__ballot(hit));
        open += (unsigned int)__popcll(__ballot(und));
    }
    const int wave = threadIdx.x / WAVE;
    if (threadIdx.x % WAVE == 0) { part[0][wave] = hits; part[1][wave] = open; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&counts[0], (unsigned long long)part[0][0] + part[0][1] + part[0][2] + part[0][3]);
        atomicAdd(&counts[1], (unsigned long long)part[1][0] + part[1][1] + part[1][2] + part[1][3]);
    }
}

}  // namespace r4r

extern "C" int r4r_rank_top1(const float *scores, int64_t rows, int C, int64_t *counts, void *stream) {
    R4R_REQUIRE(counts && rows >= 0 && C >= 2 && C <= 64, "rank_top1: counts, rows >= 0 and 2 <= C <= 64 (got %d)", C);
    if (rows == 0) return R4R_OK;
    R4R_REQUIRE(scores, "rank_top1: null scores");
    const int64_t blocks = cdiv(rows, 256);
    const unsigned grid = (unsigned)(blocks < 1024 ? blocks : 1024);
    auto *c = reinterpret_cast<unsigned long long *>(counts);
    // (the 8-byte loads of the six-column form need the rows 8-byte aligned: 24-byte rows from an 8-byte aligned base)
    if (C == 6 && reinterpret_cast<uintptr_t>(scores) % 8 == 0)
        rank_top1_kernel<6><<<grid, 256, 0, as_stream(stream)>>>(scores, rows, C, c);
    else
        rank_top1_kernel<0><<<grid, 256, 0, as_stream(stream)>>>(scores, rows, C, c);
    return check_launch("rank_top1");
}

extern "C" int r4r_deepconn_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch,
                                       int64_t launches, int64_t *built_group, int64_t *launches_done,
                                       const float *table, int64_t V, float *flat_p, float *sse_accum, void *ws,
                                       size_t ws_bytes, int T, int E, int L, float dropout_p, uint64_t seed,
                                       uint64_t offset, int conv_algo, int token_buffer, int token_alternate,
                                       float *pred_out, float *se_out, float *aux_out, void *stream) {
    (void)aux_out;
    if (int rc = check_doc_shape(loader, "deepconn_span_score", 0, T, launches_done, true)) return rc;
    R4R_REQUIRE(pred_out, "deepconn_span_score: null pred_out");
    return run_score("deepconn_span_score", loader, nb_item, first_launch, launches, built_group, launches_done, se_out,
                     as_stream(stream), [&](int64_t k, const SpanBatch &c, int64_t n) {
                         return r4r_deepconn_step(table, V, c.user_doc, c.item_doc, c.y, flat_p, nullptr, pred_out + k * n,
                                                  se_out ? se_out + k * n : nullptr, c.y ? sse_accum : nullptr, ws,
                                                  ws_bytes, n, T, E, L, dropout_p, 0, seed, offset, 1.f, conv_algo,
                                                  (token_buffer + (token_alternate ? (int)k : 0)) & 1, 0, nullptr, nullptr,
                                                  nullptr, nullptr, 0.f, 0.0, 0.0, 0.f, 0.f, 0, stream);
                     });
}

extern "C" int r4r_deepconnpp_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch,
                                         int64_t launches, int64_t *built_group, int64_t *launches_done,
                                         const float *table, int64_t V, float *flat_p, const uint64_t *rows_p,
                                         int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes, int T, int E,
                                         int L, float dropout_p, uint64_t seed, uint64_t offset, int conv_algo,
                                         int token_buffer, float *pred_out, float *se_out, float *aux_out,
                                         void *stream) {
    (void)aux_out;
    if (int rc = check_doc_shape(loader, "deepconnpp_span_score", 0, T, launches_done, true)) return rc;
    R4R_REQUIRE(pred_out, "deepconnpp_span_score: null pred_out");
    return run_score("deepconnpp_span_score", loader, nb_item, first_launch, launches, built_group, launches_done, se_out,
                     as_stream(stream), [&](int64_t k, const SpanBatch &c, int64_t n) {
                         return r4r_deepconnpp_step(table, V, c.user_doc, c.item_doc, c.uid, c.iid, c.y, flat_p, nullptr,
                                                    nullptr, nullptr, rows_p, nullptr, nullptr, n_users, n_items,
                                                    pred_out + k * n, se_out ? se_out + k * n : nullptr, nullptr, ws,
                                                    ws_bytes, n, T, E, L, dropout_p, 0, seed, offset, 1.f, conv_algo,
                                                    (token_buffer + (int)k) & 1, 0, nullptr, nullptr, 0.f, 0.0, 0.0, 0.f,
                                                    0.f, 0, stream);
                     });
}

extern "C" int r4r_narre_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch,
                                    int64_t launches, int64_t *built_group, int64_t *launches_done, const float *table,
                                    int64_t V, float *flat_p, const uint64_t *rows_p, int64_t n_users, int64_t n_items,
                                    void *ws, size_t ws_bytes, int R, int T, int E, int L, float dropout_p,
                                    uint64_t seed, uint64_t offset, int conv_algo, int token_buffer, float *pred_out,
                                    float *se_out, float *aux_out, void *stream) {
    (void)aux_out;
    if (launches_done) *launches_done = 0;
    R4R_REQUIRE(R == NB, "narre_span_score: R = %d reviews, the ring holds %d neighbour ids per rating", R, NB);
    if (int rc = check_doc_shape(loader, "narre_span_score", R, T, launches_done, true)) return rc;
    R4R_REQUIRE(pred_out, "narre_span_score: null pred_out");
    return run_score("narre_span_score", loader, nb_item, first_launch, launches, built_group, launches_done, se_out,
                     as_stream(stream), [&](int64_t k, const SpanBatch &c, int64_t n) {
                         // NARRE.py:87-96: reviewed_items = data[2], users_who_reviewed = data[1]
                         return r4r_narre_step(table, V, c.user_doc, c.item_doc, c.what, c.who, c.uid, c.iid, c.y, flat_p,
                                               nullptr, nullptr, nullptr, rows_p, nullptr, nullptr, n_users, n_items,
                                               pred_out + k * n, se_out ? se_out + k * n : nullptr, nullptr, ws, ws_bytes,
                                               n, R, T, E, L, dropout_p, 0, seed, offset, 1.f, conv_algo,
                                               (token_buffer + (int)k) & 1, 0, nullptr, nullptr, 0.f, 0.0, 0.0, 0.f, 0.f,
                                               0, stream);
                     });
}

extern "C" int r4r_transnet_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch,
                                       int64_t launches, int64_t *built_group, int64_t *launches_done,
                                       const float *table, int64_t V, float *flat_p, const uint64_t *rows_p,
                                       int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes, int T, int E, int L,
                                       int plus, float dropout_p, uint64_t seed, uint64_t offset, int conv_algo,
                                       int token_buffer, float *pred_out, float *se_out, float *aux_out,
                                       void *stream) {
    if (int rc = check_doc_shape(loader, "transnet_span_score", 0, T, launches_done, true)) return rc;
    R4R_REQUIRE(pred_out && aux_out && ws, "transnet_span_score: null pred_out / aux_out / workspace");
    return run_score(
        "transnet_span_score", loader, nb_item, first_launch, launches, built_group, launches_done, se_out,
        as_stream(stream), [&](int64_t k, const SpanBatch &c, int64_t n) {
            if (int rc = r4r_transnet_step(table, V, c.user_doc, c.item_doc, c.this_doc, c.uid, c.iid, c.y, flat_p,
                                           nullptr, nullptr, nullptr, rows_p, nullptr, nullptr, n_users, n_items,
                                           pred_out + k * n, se_out ? se_out + k * n : nullptr, nullptr, ws, ws_bytes, n,
                                           T, E, L, plus, dropout_p, 0, seed, offset, 1.f, conv_algo,
                                           (token_buffer + (int)k) & 1, 0, nullptr, nullptr, nullptr, 1, 0, 1, 0.f, 0.0,
                                           0.0, 0.f, 0.f, 0, stream))
                return rc;
            if (!c.y) return R4R_OK;                        // (no ratings: the step wrote no target SE to copy)
            const float *aux3 = reinterpret_cast<const float *>(
                static_cast<const char *>(ws) + r4r_transnet_ws_offset(n, T, E, L, plus, V, n_users, n_items, 3));
            score_aux_kernel<<<(unsigned)cdiv(n, 256), 256, 0, as_stream(stream)>>>(aux3, aux_out + k * n * 2, n);
            return check_launch("transnet_span_score(aux)");
        });
}

extern "C" int r4r_mf_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch, int64_t launches,
                                 int64_t *built_group, int64_t *launches_done, const uint64_t *p, int64_t n_users,
                                 int64_t n_items, int D, void *ws, size_t ws_bytes, float dropout_p, uint64_t seed,
                                 uint64_t offset, float *pred_out, float *se_out, float *aux_out, void *stream) {
    (void)aux_out;
    if (launches_done) *launches_done = 0;
    R4R_REQUIRE(pred_out, "mf_span_score: null pred_out");
    return run_score("mf_span_score", loader, nb_item, first_launch, launches, built_group, launches_done, se_out,
                     as_stream(stream), [&](int64_t k, const SpanBatch &c, int64_t n) {
                         return r4r_mf_step(c.uid, c.iid, c.y, p, nullptr, nullptr, n_users, n_items, D, pred_out + k * n,
                                            se_out ? se_out + k * n : nullptr, nullptr, ws, ws_bytes, n, dropout_p, 0,
                                            seed, offset, 1.f, 1, 0, 1, 0.f, 0.0, 0.0, 0.f, 0.f, 0, stream);
                     });
}

extern "C" int r4r_idnet_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch,
                                    int64_t launches, int64_t *built_group, int64_t *launches_done, int variant,
                                    float *flat_p, const uint64_t *rows_p, int64_t n_users, int64_t n_items, void *ws,
                                    size_t ws_bytes, int L, float dropout_p, uint64_t seed, uint64_t offset,
                                    float *pred_out, float *se_out, float *aux_out, void *stream) {
    (void)aux_out;
    if (launches_done) *launches_done = 0;
    R4R_REQUIRE(pred_out, "idnet_span_score: null pred_out");
    return run_score("idnet_span_score", loader, nb_item, first_launch, launches, built_group, launches_done, se_out,
                     as_stream(stream), [&](int64_t k, const SpanBatch &c, int64_t n) {
                         return r4r_idnet_step(variant, c.uid, c.iid, c.y, flat_p, nullptr, nullptr, nullptr, rows_p,
                                               nullptr, nullptr, n_users, n_items, pred_out + k * n,
                                               se_out ? se_out + k * n : nullptr, nullptr, ws, ws_bytes, n, L, dropout_p,
                                               0, seed, offset, 1.f, 1, 0, 1, 0.f, 0.0, 0.0, 0.f, 0.f, 0, stream);
                     });
}

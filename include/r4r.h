/* r4r.h -- C ABI of libr4r_hip.so, the MI355X (gfx950) rating-prediction hot path.
 *
 * The reference (noveens/reviews4rec) has no FFI: its hot path is the list of
 * ATen ops that pytorch_models/{common_pytorch_models,MF,DeepCoNN,NARRE,TransNet}.py
 * and torch.optim.Adam dispatch per training step.  Each entry point below
 * replaces one of those call sites (cited as file:line under the reference
 * root) and is what a binding written against the reference would bind.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch owns all
 *     memory); sizes are element counts unless a name ends in _bytes
 *   - fp32 data, int64 indices (the reference's LongTensor batches,
 *     data_fast.py:101-108), int32 argmax
 *   - `stream` is a hipStream_t; nothing synchronises internally, nothing
 *     allocates, every call is asynchronous and graph-capturable
 *   - return 0 on success, <0 on error; r4r_last_error() describes the last
 *     failure on the calling thread; nothing throws or aborts
 *   - thread-compatible: no hidden global state besides the error string
 */
#ifndef R4R_H
#define R4R_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define R4R_OK 0
#define R4R_ERR_ARG (-1)      /* bad shape / null pointer / unsupported size */
#define R4R_ERR_LAUNCH (-2)   /* HIP runtime refused the launch */
#define R4R_ERR_WORKSPACE (-3)/* workspace too small */

int r4r_version(void);
const char *r4r_last_error(void);

/* ------------------------------------------------------------------------
 * TextCNN tower: word gather -> conv(3 x E, pad 2) -> relu -> global max-pool
 * Replaces  nn.Embedding lookup      DeepCoNN.py:53-54, NARRE.py:95-96, TransNet.py:100-102
 *           Conv2d + relu + max_pool common_pytorch_models.py:29-31
 * The [N,T,E] gathered activations and the [N,F,T+2] conv output are never
 * written to HBM.  Two algorithms compute the same function (selection: R4R_CONV_AUTO rule in
 * DESIGN.md 4.1b; env R4R_CONV_ALGO=direct|project pins one): the direct gather-fused MFMA conv
 * over every position, or project-then-gather (projection GEMM over the batch's distinct tokens
 * + gather-add-max over positions).
 *   table  [V, E]   frozen word vectors (E % 4 == 0)
 *   idx    [N, T]   token ids in [0, V)
 *   conv_w [F, 3, E] (= Conv2d weight [F,1,3,E]),  conv_b [F],  F <= 112
 *   pooled [N, F]   max_p relu(conv)          argmax [N, F]  position p in [0,T+2) of the
 *                                              max, or -1 where pooled == 0 (no gradient)
 * ---------------------------------------------------------------------- */
size_t r4r_textcnn_ws_bytes(int64_t N, int T, int E, int F, int64_t V);
int r4r_textcnn_fwd(const float *table, int64_t V, const int64_t *idx,
                    const float *conv_w, const float *conv_b,
                    float *pooled, int32_t *argmax,
                    void *ws, size_t ws_bytes,
                    int64_t N, int T, int E, int F, void *stream);

/* The algorithm a request resolves to: `requested` R4R_CONV_AUTO / _DIRECT / _PROJECT for N documents (per
 * tower) of T words, embed size E, F filters -> R4R_CONV_DIRECT or R4R_CONV_PROJECT (the static
 * R4R_CONV_AUTO rule and the R4R_CONV_ALGO environment pin applied). */
int r4r_conv_algo(int requested, int64_t N, int T, int E, int F);

/* The request r4r_textcnn_fwd resolves its algorithm from (A/B runs and tests): R4R_CONV_AUTO (the default),
 * R4R_CONV_DIRECT or R4R_CONV_PROJECT, passed through r4r_conv_algo's rule -- the R4R_CONV_ALGO environment pin
 * still wins.  Process-wide, like r4r_gemm_form; the fused engines are not affected (they pass their own
 * conv_algo).  Returns the previous request, or R4R_ERR_ARG for any other value. */
int r4r_textcnn_algo(int requested);

/* The MEASURED rule behind the engines' automatic choice: project-then-gather's work follows the batch's
 * DISTINCT tokens, the direct conv's its positions.  `rows`: distinct tokens of a batch summed over its
 * towers (left by the gather kernel next to each tower's token counter: the int after it), `docs`:
 * documents summed over the towers, V: vocabulary.  Returns R4R_CONV_PROJECT or R4R_CONV_DIRECT by a cost
 * model fitted to MI355X measurements.  Host-side arithmetic, no device work. */
int r4r_conv_pick(int E, int T, int64_t docs, int64_t rows, int64_t V);

/* Arithmetic of the projection GEMM inside project-then-gather.  0 (default, the fp32 results every parity claim
 * refers to): fp32 operands on the fp32 MFMA.  1 (opt-in experiment): every operand split exactly
 * into two fp16 numbers (hi + lo), three f16-MFMA products per fp32 product into ONE fp32 accumulator, exact
 * power-of-two scaling from `table_maxabs` = max |word table| (frozen: computed once by the host) and
 * `weight_maxabs` = max |conv weights| over the towers (the host re-reads it every few steps; the scale keeps two
 * binades of headroom): ~2^-21 relative error per product at 16 / 3 the fp32-MFMA rate.  Mode 1 applies to the fused
 * steps (their host keeps the scales current); mode 2 also to r4r_textcnn_fwd (the caller vouches that the scales
 * describe the table and weights it passes).  Process-wide, like r4r_gemm_form. */
int r4r_gemm_math(int mode, float table_maxabs, float weight_maxabs);

/* Form of the projection GEMM inside project-then-gather (A/B runs and tests; results are bit-identical):
 * 1 = the balanced 7-row-tile form wherever its plan applies, 3 = the same plan in its A-resident form (the
 * workgroup's table rows stay in LDS for all of K, weight fragments go global -> registers, the K sweep runs once per
 * group of row tiles so that finished rows leave the chip while the rest is computed; word_embed_size <= 320, else
 * form 1), 4 = the weight-resident form (the tower's
 * 300 x E weights stay in LDS, table fragments go global -> registers, units of 16 rows x 64 columns round-robin
 * over the waves; word_embed_size <= 128, else form 3), 0 = always the 128-row tile form (its last, partial round
 * cut into column parts where that fills idle workgroups), 2 = the tile form with whole tiles only, -1 = take it
 * from the environment again (R4R_GEMM=tile / whole / balanced / ares / resident-weights pin 0 / 2 / 1 / 3 / 4;
 * unset: form 4 for word_embed_size <= 64, form 3 above). */
int r4r_gemm_form(int balanced);

/* Schedule of the gather-add-max inside the fused DeepCoNN step (A/B runs and tests; results are bit-identical).
 * 1 (default): a step that is given the next batch (same shape) also flags, on its head launch, which 128-position
 * segments of that batch are live -- not one repeated row, i.e. not the zero padding of data.py:198-199 -- and, on its
 * backward launch, writes the stable partition "live segments first" as a plan next to that batch's token state; the
 * next step's gather (tokens_ready = 1) then hands every workgroup one live and one uniform segment instead of two
 * neighbours.  The plan is used only where it applies: an even number of segments per document, at most 4,096 segments
 * per tower, at least an eighth of them uniform; everywhere else, and with 0, the gather keeps its mapping by position.
 * Process-wide, like r4r_gemm_form.  Returns the previous setting. */
int r4r_gather_plan(int on);

/* Backward of the tower w.r.t. conv weight and bias (the word table is frozen:
 * Embedding.from_pretrained, DeepCoNN.py:15 -- no dgrad exists).
 * Replaces  convolution_backward / max_pool2d_with_indices_backward /
 *           threshold_backward behind common_pytorch_models.py:29-31.
 * Only the argmax window of each (n, f) carries gradient:
 *   d_conv_w[f, j, :] = sum_n g_pooled[n, f] * table[idx[n, argmax[n,f] - 2 + j], :]
 *   d_conv_b[f]       = sum_n g_pooled[n, f]            (terms with argmax < 0 dropped)
 * Outputs are overwritten, not accumulated. */
int r4r_textcnn_wgrad(const float *table, int64_t V, const int64_t *idx,
                      const float *g_pooled, const int32_t *argmax,
                      float *d_conv_w, float *d_conv_b,
                      void *ws, size_t ws_bytes,
                      int64_t N, int T, int E, int F, void *stream);

/* ------------------------------------------------------------------------
 * Small dense layers (nn.Linear with in/out <= 256), optional fused ReLU.
 * Replaces  TextCNN.fc                 common_pytorch_models.py:37
 *           DeepCoNN.final             DeepCoNN.py:21-26,69
 *           MF.projection              MF.py:26-31,62
 *           NARRE.final                NARRE.py:38-43,123
 *           Source.project             TransNet.py:17-21,33
 *   x [N, n_in], w [n_out, n_in], b [n_out], y [N, n_out]
 * bwd: g_x may be NULL; g_w / g_b are overwritten.  With relu != 0, `y` is the
 * post-activation output saved by fwd. */
int r4r_linear_fwd(const float *x, const float *w, const float *b, float *y,
                   int64_t N, int n_in, int n_out, int relu, void *stream);
size_t r4r_linear_bwd_ws_bytes(int64_t N, int n_in, int n_out);   /* 0 for small N (ws may be NULL) */
int r4r_linear_bwd(const float *x, const float *w, const float *y, const float *g_y,
                   float *g_x, float *g_w, float *g_b, void *ws, size_t ws_bytes,
                   int64_t N, int n_in, int n_out, int relu, void *stream);

/* ------------------------------------------------------------------------
 * Dropout (nn.Dropout in train mode).  Replaces common_pytorch_models.py:37,
 * DeepCoNN.py:24, MF.py:52-53, NARRE.py:27,34,39,115-116, TransNet.py:34,58,108-109.
 * mult[i] is 0 or 1/(1-p) drawn from Philox4x32-10(seed, offset + i/4); the
 * multiplier tensor is kept for backward (g_x = g_y * mult) and so a test can
 * inject the same mask into the CPU oracle.  The reference draws from torch's
 * unseeded global RNG, so streams are not comparable. */
int r4r_dropout_fwd(const float *x, float *y, float *mult, int64_t n, float p,
                    uint64_t seed, uint64_t offset, uint64_t *offset_dev, void *stream);
/* offset_dev (nullable, DEVICE): the stream position lives in device memory: the kernel uses
 * offset + *offset_dev and *offset_dev is advanced by ceil(n/4) afterwards on the same stream,
 * so a captured hipGraph draws fresh masks on every replay. */
int r4r_counter_add(uint64_t *counter, uint64_t delta, void *stream);
int r4r_mul(const float *a, const float *b, float *out, int64_t n, void *stream);
int r4r_add(const float *a, const float *b, float *out, int64_t n, void *stream);

/* ------------------------------------------------------------------------
 * Factorisation machine head (no global bias).
 * Replaces  TorchFM.forward            common_pytorch_models.py:49-57
 *   out[b] = 0.5 * (sum_k (x V)_k^2 - sum_k (x^2 V^2)_k) + lin_w . x + lin_b
 *   x [N, n], V [n, k], lin_w [n], lin_b [1], out [N]     (n <= 512: the reference bounds neither latent_size nor
 *   the FM width -- hyper_params.py:63, DeepCoNN.py:32 reads 2 x latent_size inputs; k <= 4096)
 * bwd overwrites g_x [N,n], g_V [n,k], g_lin_w [n], g_lin_b [1]. */
int r4r_fm_fwd(const float *x, const float *V, const float *lin_w, const float *lin_b,
               float *out, int64_t N, int n, int k, void *stream);
int r4r_fm_bwd(const float *x, const float *V, const float *lin_w, const float *g_out,
               float *g_x, float *g_V, float *g_lin_w, float *g_lin_b,
               int64_t N, int n, int k, void *stream);

/* ------------------------------------------------------------------------
 * ID-embedding / bias-vector gathers and their dense gradients.
 * Replaces  nn.Embedding(user/item)    MF.py:52-53, NARRE.py:110,112,115-116, TransNet.py:108-109
 *           Parameter.gather           MF.py:45-46, DeepCoNN.py:70-71, NARRE.py:87-88
 *           embedding_dense_backward / scatter_add behind them
 *   table [R, D] (D = 1 for a bias vector), idx [n], out [n, D]
 * scatter_add zero-fills g_table [R, D] and adds every g_out row into it (the
 * reference's gradients for these tables are DENSE). */
int r4r_embed_gather(const float *table, const int64_t *idx, float *out,
                     int64_t R, int D, int64_t n, void *stream);
int r4r_embed_scatter_add(const float *g_out, const int64_t *idx, float *g_table,
                          int64_t R, int D, int64_t n, void *stream);
/* Same result, fixed summation order (the first occurrence of a row adds its later duplicates in
 * ascending entry order; no atomics): bit-identical on every run and every rank.  Used to rebuild
 * the dense gradient from the all-gathered compact (row-id, grad-row) lists under data parallelism
 * (no reference counterpart: the reference is single-process). */
int r4r_embed_scatter_add_ordered(const float *g_out, const int64_t *idx, float *g_table,
                                  int64_t R, int D, int64_t n, void *stream);

/* ------------------------------------------------------------------------
 * Rating head pieces.
 * rowdot: out[b] = sum_d a[b,d] * c[b,d]          torch.sum(user*item,-1), MF.py:57
 * bias_head: out[b] = (r ? r[b] : 0) + user_bias[uid[b]] + item_bias[iid[b]] + global_bias[0]
 *           MF.py:45-49,58,68; DeepCoNN.py:70-72; NARRE.py:87-88,124
 *           user_bias == NULL (then item_bias/uid/iid are ignored): out[b] = r[b] + global_bias[0],
 *           the 'deepconn' head  self.global_bias + fm(cat)[:, 0]  (DeepCoNN.py:65)
 * bias_head_bwd overwrites the DENSE g_user_bias [RU], g_item_bias [RI] (skipped when
 * g_user_bias == NULL) and g_global [1]  (g_r == g_out, the caller aliases it). */
int r4r_rowdot_fwd(const float *a, const float *c, float *out, int64_t N, int D, void *stream);
int r4r_rowdot_bwd(const float *a, const float *c, const float *g_out, float *g_a, float *g_c,
                   int64_t N, int D, void *stream);
int r4r_bias_head_fwd(const float *r, const float *user_bias, const float *item_bias,
                      const float *global_bias, const int64_t *uid, const int64_t *iid,
                      float *out, int64_t N, void *stream);
int r4r_bias_head_bwd(const float *g_out, const int64_t *uid, const int64_t *iid,
                      float *g_user_bias, float *g_item_bias, float *g_global,
                      int64_t RU, int64_t RI, int64_t N, void *stream);

/* ------------------------------------------------------------------------
 * NARRE review-level attention.  Replaces NARRE.attention, NARRE.py:53-64 with
 * scorer = Linear(2L->L), ReLU, Dropout, Linear(L->1) (NARRE.py:24-36):
 *   h      = relu(W0 [x ; other] + b0) * mult          (mult NULL in eval / p = 0)
 *   a      = softmax_R(w3 . h + b3)                    (padded reviews NOT masked)
 *   out[n] = sum_r a[n,r] * x[n,r,:]
 *   x, other [N, R, L]; W0 [L, 2L]; b0 [L]; w3 [L]; b3 [1]; out [N, L]
 * fwd saves h [N,R,L] (post relu, post dropout) and a [N,R] for backward.
 * bwd overwrites g_x, g_other [N,R,L], g_W0, g_b0, g_w3, g_b3; ws holds the
 * per-row scorer gradients it reduces over.   L <= 32, R <= 32. */
size_t r4r_narre_attn_ws_bytes(int64_t N, int R, int L);
int r4r_narre_attn_fwd(const float *x, const float *other, const float *W0, const float *b0,
                       const float *w3, const float *b3, const float *mult,
                       float *out, float *h_save, float *a_save,
                       int64_t N, int R, int L, void *stream);
int r4r_narre_attn_bwd(const float *x, const float *other, const float *W0, const float *w3,
                       const float *mult, const float *h_save, const float *a_save,
                       const float *g_out,
                       float *g_x, float *g_other, float *g_W0, float *g_b0, float *g_w3, float *g_b3,
                       void *ws, size_t ws_bytes,
                       int64_t N, int R, int L, void *stream);

/* ------------------------------------------------------------------------
 * Per-example squared error + its gradient for mean(SE) over `denom` examples.
 * Replaces  MSELoss.forward + torch.mean   loss.py:7-11, main.py:56-58
 *   se[b] = (out[b]-y[b])^2 ; g_out[b] = 2 (out[b]-y[b]) / denom   (g_out may be NULL) */
int r4r_mse_fwd_bwd(const float *out, const float *y, float *se, float *g_out,
                    int64_t N, float denom, void *stream);

/* TransNet transform loss  mean_n sum_l (a[n,l] - b[n,l])^2  (a = source.ir, b = target.ir).
 * Replaces  torch.mean(torch.sum(torch.pow(.., 2), -1))   TransNet.py:121
 *   a, b [N, L]; out [1]; bwd: g_out [1] -> g_a, g_b [N, L] */
int r4r_sqdist_mean_fwd(const float *a, const float *b, float *out, int64_t N, int L, void *stream);
int r4r_sqdist_mean_bwd(const float *a, const float *b, const float *g_out, float *g_a, float *g_b,
                        int64_t N, int L, void *stream);

/* ------------------------------------------------------------------------
 * Dense fused Adam over many tensors in one launch.
 * Replaces  torch.optim.Adam(lr, weight_decay).step()   main.py:94-96,60
 * (defaults betas (0.9, 0.999), eps 1e-8, L2 decay added to the gradient,
 * bias correction; every element of every listed tensor moves each step,
 * SURVEY.md fact 4).
 *   p/g/m/v : HOST arrays of `ntensor` DEVICE pointers, numel : HOST int64[ntensor] (the one
 *   exception to "every pointer is a device pointer": the tensor list is passed by value in
 *   the kernel arguments, 16 tensors per launch, so no descriptor table lives in HBM and no
 *   H2D copy happens per step).  One workgroup per r4r_adam_chunk_elems()-element chunk (1024
 *   when the whole list is under 4 M elements: latency-bound, more and shorter workgroups).
 *   g[i] == 0 means "gradient is zero" (weight decay still applies).
 *   step = 1-based step count shared by all listed tensors; or step_dev (nullable, DEVICE):
 *   a counter of COMPLETED steps in device memory -- the kernel then uses t = *step_dev + 1 and
 *   derives the bias corrections itself (for hipGraph replay; the caller advances the counter
 *   with r4r_counter_add after the launch). */
int r4r_adam_chunk_elems(void);
int r4r_adam_multi(int ntensor, const uint64_t *p, const uint64_t *g, const uint64_t *m, const uint64_t *v,
                   const int64_t *numel, float lr, double beta1, double beta2, float eps,
                   float weight_decay, int64_t step, const int64_t *step_dev, void *stream);
/* Data-parallel Adam on one flat buffer: gradient = sum over the `world` per-rank buffers of an
 * all_gather (`gathered` [world][numel], added in rank order: identical bits on every rank),
 * update as above in the same pass; g_sum (nullable) receives the summed gradient.  numel % 4 == 0,
 * 16-byte aligned buffers (the flat buffers of r4r_deepconn_layout are). */
int r4r_adam_gathered(float *p, const float *gathered, int world, float *g_sum, float *m, float *v,
                      int64_t numel, float lr, double beta1, double beta2, float eps,
                      float weight_decay, int64_t step, void *stream);
/* The same behind a device-side guard: `abort_word` (nullable, DEVICE uint32) != 0 makes the launch a no-op.  The
 * peer exchange below passes its timed_out word: slots a missing rank never filled must not be summed. */
int r4r_adam_gathered_guarded(float *p, const float *gathered, int world, float *g_sum, float *m, float *v,
                              int64_t numel, float lr, double beta1, double beta2, float eps,
                              float weight_decay, int64_t step, const uint32_t *abort_word, void *stream);

/* Device-side form of that all_gather over peer-mapped buffers (the exchange step of the data-parallel form of
 * main.py:56-60; the reference itself is single-process, main.py:407).  Every rank owns two gathered buffers
 * [world][numel] (alternating by step parity) and a flag array [world] of uint32, all zero-initialised, and has
 * them mapped by its peers:
 *   r4r_peer_segment_create: one zero-filled FINE-GRAINED device allocation of `bytes` on the current device (the
 *     flags are polled while peers write them: coarse-grained memory promises visibility at kernel boundaries only)
 *     and its 64-byte IPC handle, which the host ships to the peers by any means it has;
 *     r4r_peer_segment_open maps a peer's handle (-> *ptr), _close unmaps it, _destroy frees one's own segment.
 *   r4r_peer_push: copies `src` [numel] into slot `rank` of every rank's gathered buffer (peer_dst[r] = rank r's
 *     buffer of this step's parity, device pointers as uint64), then -- once every workgroup's stores are fenced at
 *     system scope -- writes `epoch` (the 1-based step) to element `rank` of every rank's flag array
 *     (peer_flags[r]).  `arrive`: one zero-initialised uint32 in this rank's memory.  numel % 4 == 0, 16-byte aligned.
 *     With `wait_flags` (MY flag array) the same launch then waits as r4r_peer_wait does: the exchange is one launch.
 *   r4r_peer_wait: one wave spins until all `world` elements of MY flag array have reached `epoch`, at most
 *     `timeout_s` seconds (then *timed_out = 1 + the missing rank, and the launch ends: the caller checks it).
 * r4r_adam_gathered on the buffer then sums the slots in rank order: identical bits on every rank.  world <= 16. */
int r4r_peer_segment_create(int64_t bytes, void **ptr, uint8_t *handle);
int r4r_peer_segment_open(const uint8_t *handle, void **ptr);
int r4r_peer_segment_close(void *ptr);
int r4r_peer_segment_destroy(void *ptr);
int r4r_peer_push(const float *src, int64_t numel, const uint64_t *peer_dst, const uint64_t *peer_flags,
                  uint32_t *arrive, int rank, int world, uint32_t epoch, const uint32_t *wait_flags,
                  uint32_t *timed_out, double timeout_s, void *stream);
int r4r_peer_wait(const uint32_t *flags, int world, uint32_t epoch, uint32_t *timed_out, double timeout_s, void *stream);


/* ------------------------------------------------------------------------
 * Fused DeepCoNN step ('deepconn' mode): the whole of DeepCoNN.forward
 * (DeepCoNN.py:37-66) + MSELoss/mean (loss.py:7-11, main.py:56-58) + backward in
 * ONE call that enqueues 4 or 5 kernels (both towers share every launch; r4r_deepconn_tail).
 * Replaces, per training step, every ATen op main.py:32,56-59 dispatches.
 *
 * The trainable parameters of this mode live in ONE flat fp32 buffer; slot i of
 * r4r_deepconn_layout() (HOST out-arrays of r4r_deepconn_nparam() entries, offsets
 * in floats, 16-byte aligned) is, in order:
 *   user_conv.convs.0.weight, user_conv.convs.0.bias, user_conv.fc.weight,
 *   user_conv.fc.bias, item_conv.(same four), fm.V, fm.lin.weight, fm.lin.bias,
 *   global_bias            (`final`, user_bias, item_bias are unused in this mode,
 *                           DeepCoNN.py:64-66, and are not part of the buffer)
 * flat_g has the same layout and is OVERWRITTEN with d mean(SE)/d param, where the
 * mean is over 1/inv_denom examples (pass 1/B_global under data parallelism).
 *   flat_g == NULL : forward only (eval, or y == NULL for pure prediction)
 *   training != 0  : dropout(p) on the FC outputs, Philox4x32-10(seed, offset + b*2L + i)
 *   conv_algo      : R4R_CONV_AUTO | R4R_CONV_DIRECT (gather-fused MFMA conv over every position)
 *                    | R4R_CONV_PROJECT (projection GEMM over the batch's distinct tokens, then a
 *                    gather-add-max over positions; same function, different summation order)
 *   token_buffer   : which of the two token-state buffers of the workspace this step uses (0/1)
 *   tokens_ready   : != 0 when that buffer already holds this batch's compacted tokens
 *                    (prepared by r4r_deepconn_tokens or by the previous step, below)
 *   next_user_idx / next_item_idx (both or neither; training steps only): the NEXT batch of the
 *                    same B and T.  Its token state is prepared into buffer token_buffer ^ 1; call
 *                    the next step with that buffer and tokens_ready = 1.  Which launch carries what:
 *                    four-launch step (r4r_deepconn_tail() == 1): segment flags AND token marks on the
 *                    head launch, plan scan and compaction on the backward launch; five-launch step:
 *                    segment flags on the head launch, plan scan and marks on the backward launch,
 *                    compaction on the gradient-reduce launch.  The state left behind is the same.
 *   flat_m / flat_v (both or neither; layout of flat_p): when given, the step is also the
 *                    optimiser -- torch.optim.Adam(lr, betas, eps, weight_decay) update number
 *                    adam_step (1-based) of flat_p in place (main.py:94-96,60), done by the launch
 *                    that finishes the gradients; flat_g still receives the gradients.  Leave NULL
 *                    under data parallelism (all-reduce flat_g, then r4r_adam_multi).
 *   pred [B], se [B] (se required when y != NULL); sse_accum (nullable device scalar)
 *   is incremented by sum_b se[b] -- the host's running metric (main.py:57) without a
 *   per-step device->host sync. */
#define R4R_CONV_AUTO 0
#define R4R_CONV_DIRECT 1
#define R4R_CONV_PROJECT 2
int r4r_deepconn_nparam(void);
int r4r_deepconn_layout(int E, int L, int64_t *offsets, int64_t *sizes, int64_t *total);
size_t r4r_deepconn_ws_bytes(int64_t B, int T, int E, int L, int64_t V);
size_t r4r_deepconn_ws_mult_offset(int64_t B, int T, int E, int L, int64_t V);   /* [B,2L] dropout multipliers (tests) */
size_t r4r_deepconn_ws_count_offset(int64_t B, int T, int E, int L, int64_t V, int tower, int buffer);   /* token counter of (tower, token buffer): int[0] live count, int[1] the count the last gather consumed, int[2] whether the last gather that was given a segment plan followed it */
size_t r4r_deepconn_ws_partials_offset(int64_t B, int T, int E, int L, int64_t V, int tower, int which);   /* (tests) the tower's conv partials [B, tiles, 112]: which = 0 pmax, 1 parg */
size_t r4r_deepconn_ws_plan_offset(int64_t B, int T, int E, int L, int64_t V, int tower, int buffer, int which);   /* (tests) the gather's segment plan (r4r_gather_plan) of (tower, token buffer): which = 0 perm int[B tiles], 1 plan_ready int[1], 2 live */
size_t r4r_deepconn_ws_state_offset(int64_t B, int T, int E, int L, int64_t V, int tower, int buffer, int which);   /* (tests) token state of (tower, token buffer): which = 0 flags int[V + 4], 1 slot int[V + 4], 2 list int[count]; 3 = the tower's pooling argmax int[B, 100] (buffer ignored) */
int r4r_deepconn_step(const float *table, int64_t V, const int64_t *user_idx, const int64_t *item_idx,
                      const float *y, float *flat_p, float *flat_g,
                      float *pred, float *se, float *sse_accum,
                      void *ws, size_t ws_bytes,
                      int64_t B, int T, int E, int L,
                      float dropout_p, int training, uint64_t seed, uint64_t offset,
                      float inv_denom, int conv_algo, int token_buffer, int tokens_ready,
                      const int64_t *next_user_idx, const int64_t *next_item_idx,
                      float *flat_m, float *flat_v, float lr, double beta1, double beta2, float eps,
                      float weight_decay, int64_t adam_step, void *stream);
/* Tail of a DeepCoNN training step (A/B runs and tests; results are bit-identical).  1 (default): wherever the shape
 * allows, the step is FOUR launches -- GEMM, gather, head, backward -- and the backward launch finishes every gradient
 * sum and takes every Adam step itself (main.py:59-60): one workgroup per (tower, filter, tap) of the conv gradient
 * holds all batch splits of its row, so no partial sum leaves the chip and no workgroup waits for another.  0: always
 * the five-launch step, whose gradient-reduce launch sums the splits' partials and runs Adam (R4R_TAIL=old in the
 * environment starts a process with 0).  Process-wide, like r4r_gemm_form.  Returns the previous setting.
 * r4r_deepconn_tail(B, E, L) -> 1 where a training step of that batch size, word_embed_size and latent_size takes the
 * four-launch form under the current switch, else 0.  A pure function of its arguments and the switch: the batch must
 * be at most 256 ratings, (batch splits) x E / 4 at most 1,024 (one thread per float4 column and split: E = 300 at
 * B = 128 is 8 x 76; E = 768 at B = 128 is not taken), latent_size at most 64. */
int r4r_deepconn_tail_fold(int on);
int r4r_deepconn_tail(int64_t B, int E, int L);
/* Token compaction of a batch (distinct tokens -> dense rows) into token-state buffer 0 or 1 of the
 * workspace.  It depends only on the indices, so the caller may run it for batch k+1 on another
 * stream while step k computes, and then pass token_buffer / tokens_ready = 1 to step k+1
 * (otherwise the step does it itself).  The workspace must be zero-filled when created; the
 * kernels keep the flag / count words zero between calls. */
int r4r_deepconn_tokens(const int64_t *user_idx, const int64_t *item_idx, void *ws, size_t ws_bytes,
                        int64_t B, int T, int E, int L, int64_t V, int conv_algo, int token_buffer,
                        int discard, void *stream);   /* discard != 0: reset a prepared but unused buffer */

/* ------------------------------------------------------------------------
 * Live kernel timing for bench.py's roofline leg (no reference counterpart: the
 * reference has no profiler hooks).  When enabled, each
 * instrumented entry point brackets its dominant kernel -- only that kernel --
 * with hipEvents (recycled from a pool) on the launch stream; read() synchronises and
 * accumulates.  Each instrumented launch costs two event records, so bench.py instruments only
 * the kernels its roofline needs.
 * `total_ms` and `count` are HOST pointers. */
#define R4R_TIMING_TEXTCNN_FWD 0    /* textcnn_fwd_kernel (the MFMA conv tile kernel) */
#define R4R_TIMING_TEXTCNN_WGRAD 1  /* textcnn_wgrad_kernel */
#define R4R_TIMING_ADAM 2           /* adam_multi_kernel */
#define R4R_TIMING_PROJ_GEMM 3      /* proj_gemm_kernel (projection of the batch's distinct tokens) */
#define R4R_TIMING_PROJ_GATHER 4    /* proj_gather_max_kernel (gather-add-max over positions) */
#define R4R_TIMING_SLOTS 8
int r4r_timing_enable(int slot_mask);   /* bit i instruments slot i; 0 switches timing off */
int r4r_timing_read(int slot, double *total_ms, int64_t *count, int reset);

/* ------------------------------------------------------------------------
 * Fused native step for the ID-only recommenders: model_type 'MF_dot' and 'bias_only'
 * Replaces, per training step, MF.forward (MF.py:39-58: user/item bias gathers, the two
 * ID-embedding gathers + dropout, the row dot product), MSELoss (loss.py:7-11), loss.backward()
 * and torch.optim.Adam.step() (main.py:56-60,94-96) by TWO launches.  The dense gradient of an
 * ID table is never materialised: gradient rows stay compact ([B, D]) and the Adam sweep treats a
 * row no rating touched as gradient zero (24 B/element instead of 28 + a zero fill); a touched row
 * is updated by the wave of its first rating, which sums the row's entries in a fixed order
 * (deterministic, no atomics).
 *   p / m / v : HOST arrays of 5 DEVICE pointers -- user_embedding.weight [n_users, D],
 *               item_embedding.weight [n_items, D], user_bias [n_users], item_bias [n_items],
 *               global_bias [1] (n_users = total_users + 1, n_items = total_items + 1, MF.py:14-24);
 *               the two table entries are ignored when D == 0 ('bias_only').
 *               m == v == NULL: forward only (pred, and se when y is given).
 *   dropout   : Philox4x32-10(seed, offset + b*2D + d) for the user row, + D for the item row
 *   adam_step : 1-based update count; also tags the rows this step touched (workspace)
 *   ws        : r4r_mf_ws_bytes; its first r4r_mf_ws_persist_bytes (per-row step tags and the
 *               owner-election slots) must be ZERO on first use and are kept consistent by the
 *               kernels as long as adam_step only grows -- allocate once, zero once; a caller
 *               that switches buffers (another B) carries that head over.
 *   B <= 16384 for training steps.  sse_accum (nullable) += sum_b se[b] on training steps. */
size_t r4r_mf_ws_bytes(int64_t B, int D, int64_t n_users, int64_t n_items);
size_t r4r_mf_ws_persist_bytes(int64_t B, int D, int64_t n_users, int64_t n_items);
size_t r4r_mf_ws_mult_offset(int64_t B, int D, int64_t n_users, int64_t n_items);   /* [B,2D] dropout multipliers (tests) */
size_t r4r_mf_ws_grad_offset(int64_t B, int D, int64_t n_users, int64_t n_items, int which);   /* 0: user rows [B,D], 1: item rows, 2: d loss/d pred [B] (tests) */
int r4r_mf_step(const int64_t *uid, const int64_t *iid, const float *y,
                const uint64_t *p, const uint64_t *m, const uint64_t *v,
                int64_t n_users, int64_t n_items, int D,
                float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes, int64_t B,
                float dropout_p, int training, uint64_t seed, uint64_t offset, float inv_denom,
                int sweep_period, int64_t sweep_base, int sweep_all,
                float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                void *stream);

/* sweep_period P in 2..8: the Adam sweep over the two ID tables, temporally blocked on a SCHEDULE (round 4).  A table
 * element no rating names goes through the same gradient-zero update whether it is applied now or together with the
 * next ones (it reads nothing but its own p, m, v and the step's two bias corrections), so chunk c of 1,024 table
 * elements is visited only at the steps s with (c % P + c / P + s) % P == 0 -- one chunk of every P consecutive
 * ones per step, a launch of exactly the due chunks -- and then takes all its pending updates in order, each with its
 * own step's scalars: the fp32 operations per element are those of the dense sweep (bit-identical tables and
 * moments: tests/test_gpu_full_size.py), the traffic a P-th.  Nothing is announced and no per-chunk state is kept:
 * the step of a chunk's last visit is a function of (c, step), a row a rating names is current through
 * max(sweep_base, that visit, the row's own last update [kept per row in ws]), and whoever needs it newer applies the
 * missing updates on the way -- the forward in registers, the row's entry wave before its gradient update.
 *   sweep_base : a completed step through which EVERY element is current (0 before the first step).  The caller keeps
 *                it: it becomes adam_step after a call with sweep_all = 1 or P = 1 and after r4r_mf_rows_flush, and
 *                stays otherwise.  At most 8 updates may be pending anywhere (guaranteed while every step since
 *                sweep_base ran this function with the same P); the int at r4r_mf_ws_flag_offset is set if not.
 *   sweep_all  : 1 = visit every chunk now (the plain dense sweep, applying whatever is pending under the schedule
 *                (P, sweep_base)); required on the step that changes P.
 * r4r_mf_rows_flush(adam_step = the last COMPLETED step) brings every element up to date without a step; a forward-only
 * r4r_mf_step (m == NULL) and anything else that reads the tables needs it first.  16-byte aligned tables; others
 * are swept densely every step. */
int r4r_mf_rows_flush(const uint64_t *p, const uint64_t *m, const uint64_t *v,
                      int64_t n_users, int64_t n_items, int D, void *ws, size_t ws_bytes, int64_t B,
                      int sweep_period, int64_t sweep_base,
                      float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                      void *stream);
size_t r4r_mf_ws_flag_offset(int64_t B, int D, int64_t n_users, int64_t n_items);

/* accum[0] += sum of se[0 .. n) in a fixed order (the running train metric of main.py:57, kept on the device). */
int r4r_sse_accumulate(const float *se, int64_t n, float *accum, void *stream);

/* ---- MF under data parallelism: one process per GPU, replicated tables.
 * r4r_mf_grad: this rank's forward + compact gradient rows into one packed `block`
 *   (r4r_mf_dp_block_bytes(B_pad, D) bytes: uid32 [B_pad] | iid32 | g | gu [B_pad, D] | gi; entries
 *   past this rank's B carry id -1: ragged shards).  inv_denom = 1 / B_global.
 * The caller all_gathers the blocks (rank order), then every rank calls
 * r4r_mf_apply(blocks [world], ...): row tags + owner election over the gathered entries, then the
 *   same tagged sweep as r4r_mf_step -- identical bits on every rank, and identical to the
 *   single-process step on the concatenated batch.  ws: r4r_mf_ws_bytes(world * B_pad, ...), zeroed
 *   once; world * B_pad <= 1,048,576 (csrc/mf_engine.hip: MF_MAX_B_STEP, r4r_mf_step's own limit -- owners come from
 *   the election slots, ids from global memory; main.native_step_limits admits the same global batch). */
size_t r4r_mf_dp_block_bytes(int64_t B_pad, int D);
int r4r_mf_grad(const int64_t *uid, const int64_t *iid, const float *y, const uint64_t *p,
                const uint64_t *m, const uint64_t *v,
                int64_t n_users, int64_t n_items, int D, float *pred, float *se, void *block, float *mult,
                int64_t B, int64_t B_pad, float dropout_p, int training, uint64_t seed, uint64_t offset,
                float inv_denom, void *ws, int sweep_period, int64_t sweep_base,
                float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                void *stream);
int r4r_mf_apply(const void *blocks, int world, int64_t B_pad, const uint64_t *p, const uint64_t *m,
                 const uint64_t *v, int64_t n_users, int64_t n_items, int D, void *ws, size_t ws_bytes,
                 int sweep_period, int64_t sweep_base, int sweep_all,
                 const float *se, int64_t se_n, float *sse_accum,
                 float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                 void *stream);
/* se [se_n] / sse_accum (nullable): sse_accum[0] += the sum of THIS rank's se in a fixed order (the running train metric
 * of main.py:57), on the launch's global-bias workgroup instead of a launch of its own.
 * The scheduled sweep under data parallelism: r4r_mf_apply(sweep_period, sweep_base, sweep_all) -- the SAME values on
 * every rank -- is r4r_mf_step's sweep over the gathered entries; r4r_mf_grad(m, v, ws = r4r_mf_apply's workspace,
 * the same schedule and optimiser scalars; all NULL / ignored when nothing can be pending) reads the rows its ratings
 * name as of step adam_step - 1.  r4r_mf_rows_flush on every rank before anything else reads the tables.
 * Up to 2,048 gathered entries r4r_mf_apply is ONE launch: its workgroups read the ids out of the blocks and find the
 * rows the step names themselves (beyond, a registering launch runs first).
 *
 * The same step with NO collective call -- the exchange rides on the two launches, over peer-mapped memory (the
 * segments, flags and epochs of r4r_peer_* below; one process per GPU on an xGMI mesh):
 * r4r_mf_grad_push: r4r_mf_grad whose block goes straight into slot `rank` of EVERY rank's gathered buffer
 *   (peer_dst[r] = rank r's buffer of this epoch's parity, world slots of r4r_mf_dp_block_bytes each); the launch's last
 *   workgroup raises flags[r][rank] = epoch on every rank (system-scope release).  arrive: one zeroed uint32 of this rank.
 * r4r_mf_apply_peer: r4r_mf_apply on this rank's gathered buffer, every workgroup first waiting (bounded by
 *   timeout_s; *timed_out = 1 + the missing rank otherwise) until all `world` flags of wait_flags (THIS rank's flag
 *   array) have reached `epoch`.  world * B_pad <= 2,048. */
int r4r_mf_grad_push(const int64_t *uid, const int64_t *iid, const float *y, const uint64_t *p,
                     const uint64_t *m, const uint64_t *v,
                     int64_t n_users, int64_t n_items, int D, float *pred, float *se, float *mult,
                     int64_t B, int64_t B_pad, float dropout_p, int training, uint64_t seed, uint64_t offset,
                     float inv_denom, void *ws, int sweep_period, int64_t sweep_base,
                     float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                     const uint64_t *peer_dst, const uint64_t *peer_flags, uint32_t *arrive, int rank, int world,
                     uint32_t epoch, void *stream);
int r4r_mf_apply_peer(const void *blocks, int world, int64_t B_pad, const uint64_t *p, const uint64_t *m,
                      const uint64_t *v, int64_t n_users, int64_t n_items, int D, void *ws, size_t ws_bytes,
                      int sweep_period, int64_t sweep_base, int sweep_all,
                      const float *se, int64_t se_n, float *sse_accum,
                      float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                      const uint32_t *wait_flags, uint32_t epoch, uint32_t *timed_out, double timeout_s,
                      void *stream);

/* ---- data parallel: the glue around the step's ONE all_gather of the ranks' compact entries (csrc/dp_pack.hip).
 * A family's entries are `nfields` arrays of `widths[f]` 4-byte units per rating (int64 ids: 2; d loss / d pred: 1; a
 * gradient row of an ID table: its width).  r4r_dp_pack copies this rank's n entries of every field into one block
 * (r4r_dp_block_bytes; entries n .. B_pad - 1 are padding: all ones where pad_ones[f] -- an int64 id of -1 --, zero
 * elsewhere); the caller all_gathers the blocks (rank order); r4r_dp_unpack writes field f of all ranks, rank-major,
 * to dst[f] [world * B_pad, widths[f]]: the arrays the r4r_*_rows_apply launches take.  At most 8 fields. */
size_t r4r_dp_block_bytes(int nfields, const int *widths, int64_t B_pad);
int r4r_dp_pack(int nfields, const uint64_t *src, const int *widths, const int *pad_ones, int64_t n,
                int64_t B_pad, void *block, void *stream);
int r4r_dp_unpack(int nfields, const uint64_t *dst, const int *widths, const void *blocks, int world,
                  int64_t B_pad, void *stream);

/* ---- fused native step for NARRE (pytorch_models/NARRE.py:10-124)
 * Replaces, per training step: the word gathers + TextCNN over the B*R review documents of each
 * side, TextCNN's FC + dropout, both attention scorers + softmax (NARRE.py:53-64), the four
 * ID-embedding gathers, the interaction, `final`, the bias head, MSELoss (loss.py:7-11),
 * loss.backward() and torch.optim.Adam.step() (main.py:56-60,94-96) -- five launches.
 *   user_reviews / item_reviews [B, R, T] token ids; reviewed_items / users_who_reviewed [B, R]
 *   (R = narre_num_reviews = the neighbour count of data.py:274-279); uid / iid [B].
 *   flat_p / flat_g / flat_m / flat_v : the DENSE parameters in the layout of r4r_narre_layout
 *     (21 slots, 16-byte aligned): user_conv.convs.0.weight, .bias, user_conv.fc.weight, .bias,
 *     item_conv.(same four), attention_scorer_user.0.weight, .0.bias, .3.weight, .3.bias,
 *     attention_scorer_item.(same four), final.1.weight, .1.bias, .3.weight, .3.bias, global_bias.
 *     flat_g == NULL: forward only.
 *   rows_p / rows_m / rows_v : HOST arrays of 4 DEVICE pointers -- user_embedding.weight
 *     [n_users, L], item_embedding.weight [n_items, L], user_bias [n_users], item_bias [n_items]
 *     (n_users = total_users + 2, n_items = total_items + 2: NARRE.py:17-18,44-45).  Their dense
 *     gradients are never materialised (compact rows + a tagged Adam sweep, as r4r_mf_step).
 *   dropout: Philox4x32-10(seed, offset + b*(4RL+3L) + k), k = site-major: user_conv.dropout [R,L],
 *     item_conv.dropout, attention_scorer_user.2, attention_scorer_item.2, dropout.user [L],
 *     dropout.item, final.0.
 *   token_buffer / tokens_ready / next_*_reviews / conv_algo: as r4r_deepconn_step.
 *   ws: r4r_narre_ws_bytes, ZERO on first use (row tags, token flags, gradient-row padding). */
int r4r_narre_nparam(void);
int r4r_narre_layout(int E, int L, int64_t *offsets, int64_t *sizes, int64_t *total);
size_t r4r_narre_ws_bytes(int64_t B, int R, int T, int E, int L, int64_t V, int64_t n_users, int64_t n_items);
size_t r4r_narre_ws_offset(int64_t B, int R, int T, int E, int L, int64_t V, int64_t n_users, int64_t n_items,
                           int which);   /* 0 dropout multipliers, 1/2 compact rows user/item, 3/4 their ids, 5 d loss/d pred (tests);
                                         6 + 2*tower + buffer: compaction counter of a token buffer (zero the int to discard
                                         a prepared-but-unused token state) */
int r4r_narre_step(const float *table, int64_t V,
                   const int64_t *user_reviews, const int64_t *item_reviews,
                   const int64_t *reviewed_items, const int64_t *users_who_reviewed,
                   const int64_t *uid, const int64_t *iid, const float *y,
                   float *flat_p, float *flat_g, float *flat_m, float *flat_v,
                   const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                   int64_t n_users, int64_t n_items,
                   float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes,
                   int64_t B, int R, int T, int E, int L,
                   float dropout_p, int training, uint64_t seed, uint64_t offset, float inv_denom,
                   int conv_algo, int token_buffer, int tokens_ready,
                   const int64_t *next_user_reviews, const int64_t *next_item_reviews,
                   float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                   void *stream);

/* Data parallel: r4r_narre_step with flat_m == NULL computes gradients only (flat_g; the compact ID entries
 * at r4r_narre_ws_offset 1..5); after the exchange -- all-reduce flat_g + r4r_adam_multi, all_gather of the
 * ranks' entries -- this updates the two ID tables and bias vectors from ALL ranks' entries in the order
 * given (ids -1 pad ragged shards).  g_entry: an entry's bias gradient (d loss / d pred for a rating's own
 * user / item entry, 0 for a neighbour entry).  Same `ws` and shape arguments as the step.  entries <= 16384. */
int r4r_narre_rows_apply(const int64_t *gid0, const int64_t *gid1, const float *grow0, const float *grow1,
                         const float *g_entry, int64_t entries,
                         const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                         int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes,
                         int64_t B, int R, int T, int E, int L, int64_t V,
                         float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                         void *stream);
/* The same update with one exchange and no glue launches (world * B_pad * (1 + R) <= 16,384 entries, latent_size <= 32):
 * r4r_narre_dp_block packs this rank's entries of the LAST gradients-only r4r_narre_step on `ws` into `block`
 *   (r4r_narre_dp_block_bytes(B_pad, R, L) bytes: ids as int32, an entry's bias gradient, the gradient rows; the B_pad
 *   self entries first, then the neighbour entries; entries past the rank's own carry id -1), the caller all_gathers
 *   the blocks (rank order) and every rank calls
 * r4r_narre_rows_apply_blocks(blocks [world], ...): r4r_narre_rows_apply straight over the blocks, entries in (rank,
 *   in-block) order on every rank. */
size_t r4r_narre_dp_block_bytes(int64_t B_pad, int R, int L);
int r4r_narre_dp_block(void *ws, size_t ws_bytes, int64_t B, int R, int T, int E, int L, int64_t V,
                       int64_t n_users, int64_t n_items, void *block, int64_t B_pad, void *stream);
int r4r_narre_rows_apply_blocks(const void *blocks, int world, int64_t B_pad,
                                const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                                int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes,
                                int64_t B, int R, int T, int E, int L, int64_t V,
                                float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                                void *stream);

/* The same for ANY number of entries (a data-parallel step at a global batch of 8,192 gathers 90,112 entries per
 * table; a single-process step beyond the fused launch's 4,096): the named rows go through r4r_rows_apply_large
 * (below), the rows nobody names through the same tagged sweep.  `scratch`: r4r_rows_large_ws_bytes(entries) bytes. */
int r4r_narre_rows_apply_large(const int64_t *gid0, const int64_t *gid1, const float *grow0, const float *grow1,
                               const float *g_entry, int64_t entries,
                               const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                               int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes,
                               int64_t B, int R, int T, int E, int L, int64_t V,
                               float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                               void *scratch, size_t scratch_bytes, void *stream);

/* Dense-Adam update (torch.optim.Adam as at main.py:94-96) of the rows of ONE ID table [rows, W] -- and, with bp, of
 * its bias vector [rows] -- that `entries` compact entries name: a row's gradient is the sum of grads[e, :] over the
 * entries e with ids[e] == row (ids outside 0..rows-1 are padding), its bias gradient the sum of gbias[e] (nullable:
 * zero); rows no entry names are NOT touched (the caller's sweep).  Any number of entries; deterministic (no
 * floating-point atomics, no scheduling-dependent order): replicas applying the same entries hold the same bits.
 * W <= 1024.  `scratch`: r4r_rows_large_ws_bytes(entries) bytes of device memory, contents irrelevant. */
size_t r4r_rows_large_ws_bytes(int64_t entries);
int r4r_rows_apply_large(const int64_t *ids, const float *grads, const float *gbias, int64_t entries, int W,
                         float *p, float *m, float *v, float *bp, float *bm, float *bv, int64_t rows,
                         void *scratch, size_t scratch_bytes,
                         float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                         void *stream);

/* ---- fused native step for DeepCoNN++ (DeepCoNN.py:37-72, model_type 'deepconn++'): the two
 * TextCNN towers, `final` = Linear(2L, L) -> ReLU -> Dropout -> Linear(L, 1), user / item / global
 * bias.  Same structure and arguments as r4r_narre_step; user_idx / item_idx [B, T] as in
 * r4r_deepconn_step.  Flat layout (13 slots, r4r_deepconnpp_layout): user_conv.convs.0.weight, .bias,
 * user_conv.fc.weight, .bias, item_conv.(same four), final.0.weight, final.0.bias, final.3.weight,
 * final.3.bias, global_bias.  rows_p / rows_m / rows_v: HOST arrays of 2 DEVICE pointers -- user_bias
 * [n_users], item_bias [n_items] (n = total + 2).  Dropout draws per rating: user_conv.dropout [L],
 * item_conv.dropout [L], final.2 [L] at Philox counter offset + b*3L + k.  (The `fm` module the
 * reference also constructs is unused in this mode and never trained.) */
int r4r_deepconnpp_nparam(void);
int r4r_deepconnpp_layout(int E, int L, int64_t *offsets, int64_t *sizes, int64_t *total);
size_t r4r_deepconnpp_ws_bytes(int64_t B, int T, int E, int L, int64_t V, int64_t n_users, int64_t n_items);
size_t r4r_deepconnpp_ws_offset(int64_t B, int T, int E, int L, int64_t V, int64_t n_users, int64_t n_items,
                                int which);   /* 0 dropout multipliers [B,3L], 5 d loss/d pred, 6 + 2*tower + buffer: token counter */
int r4r_deepconnpp_step(const float *table, int64_t V, const int64_t *user_idx, const int64_t *item_idx,
                        const int64_t *uid, const int64_t *iid, const float *y,
                        float *flat_p, float *flat_g, float *flat_m, float *flat_v,
                        const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                        int64_t n_users, int64_t n_items,
                        float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes,
                        int64_t B, int T, int E, int L,
                        float dropout_p, int training, uint64_t seed, uint64_t offset, float inv_denom,
                        int conv_algo, int token_buffer, int tokens_ready,
                        const int64_t *next_user_idx, const int64_t *next_item_idx,
                        float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                        void *stream);

/* Data parallel: r4r_deepconnpp_step with flat_m == NULL computes gradients only (flat_g; d loss / d pred
 * at r4r_deepconnpp_ws_offset 5); after the exchange -- all-reduce flat_g + r4r_adam_multi, all_gather of
 * the ranks' (uid, iid, d loss / d pred), ids -1 padding ragged shards -- this updates the two ID bias
 * vectors from ALL ranks' ratings (same `ws` and shape arguments as the step).  B_all <= 16384. */
int r4r_deepconnpp_rows_apply(const int64_t *uid_all, const int64_t *iid_all, const float *g_all, int64_t B_all,
                              const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                              int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes,
                              int64_t B, int T, int E, int L, int64_t V,
                              float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                              void *stream);

/* ---- fused native step for TransNet / TransNet++ (TransNet.py:9-122; the three-optimiser step of
 * main.py:26-53 with utils.init_transnet_optim, utils.py:70-92).  Three TextCNN towers (user
 * documents, item documents, the review being rated: user_idx / item_idx / this_idx [B, T]) and
 * three losses from one forward -- target MSE -> target.*, transform loss mean ||s_ir - t_ir||^2 ->
 * source.*, source MSE -> source_fm.* and (TransNet++, plus = 1) the ID vectors.  The gradient each
 * of the reference's three optimisers consumes is that of its own loss on its own parameter group
 * at the pre-step weights, so the step is one backward with three disjoint groups and -- the three
 * Adams sharing lr, weight decay and step count -- one flat Adam (csrc/transnet_engine.hip has the
 * argument; the reference-generated trajectories pin it).
 * Flat layout (22 slots, r4r_transnet_layout): source.user_conv.convs.0.weight, .bias,
 * source.item_conv.convs.0.(same), target.conv.convs.0.(same), source.user_conv.fc.weight, .bias,
 * source.item_conv.fc.(same), target.conv.fc.(same), source.project.0.weight, .bias,
 * source.project.2.weight, .bias, source_fm.V, source_fm.lin.weight, .bias, target.fm.V,
 * target.fm.lin.weight, .bias.  rows_p / rows_m / rows_v: HOST arrays of 2 DEVICE pointers --
 * user_embedding.weight [n_users, 5], item_embedding.weight [n_items, 5] (TransNet++; NULL otherwise).
 * pred / se: the SOURCE prediction and its squared error (what main.py:57 sums); sse_accum (3 floats,
 * nullable) += [sum of se, this batch's mean target SE, this batch's transform loss]; the workspace
 * holds per rating (r4r_transnet_ws_offset which = 3) the target prediction, its squared error and
 * ||s_ir - t_ir||^2.  Dropout draws per rating at Philox counter offset + b*(5L+10) + k:
 * source.user_conv.dropout [L], source.item_conv.dropout [L], target.conv.dropout [L],
 * source.dropout [L], target.dropout [L], dropout.user [5], dropout.item [5] (plain TransNet has no ID
 * vectors: its last ten positions are drawn and recorded in the workspace's [B, 5L+10] multipliers like
 * the others, and no site consumes them). */
int r4r_transnet_nparam(void);
int r4r_transnet_layout(int E, int L, int plus, int64_t *offsets, int64_t *sizes, int64_t *total);
size_t r4r_transnet_ws_bytes(int64_t B, int T, int E, int L, int plus, int64_t V, int64_t n_users, int64_t n_items);
size_t r4r_transnet_ws_offset(int64_t B, int T, int E, int L, int plus, int64_t V, int64_t n_users, int64_t n_items,
                              int which);   /* 0 dropout multipliers, 1 / 2 ID-vector gradient rows [B,5], 3 aux [B,3], 4 size of the persistent head, 5 the broken-schedule flag (int), 6 + 2*tower + buffer: token counter */
int r4r_transnet_step(const float *table, int64_t V,
                      const int64_t *user_idx, const int64_t *item_idx, const int64_t *this_idx,
                      const int64_t *uid, const int64_t *iid, const float *y,
                      float *flat_p, float *flat_g, float *flat_m, float *flat_v,
                      const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                      int64_t n_users, int64_t n_items,
                      float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes,
                      int64_t B, int T, int E, int L, int plus,
                      float dropout_p, int training, uint64_t seed, uint64_t offset, float inv_denom,
                      int conv_algo, int token_buffer, int tokens_ready,
                      const int64_t *next_user_idx, const int64_t *next_item_idx, const int64_t *next_this_idx,
                      int sweep_period, int64_t sweep_base, int sweep_all,
                      float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                      void *stream);

/* The ID-vector sweep, temporally blocked on a schedule (TransNet++; the contract is r4r_mf_step's, spelled out
 * there).  torch.optim.Adam moves EVERY row of user_embedding / item_embedding every step (main.py:94-96: weight
 * decay, decaying moments), 24 bytes of traffic per element -- but an element no rating of the batch names goes
 * through the same gradient-zero update whether it is applied now or together with the next few.  With
 * sweep_period P in 2..8 a chunk of 1,024 table elements is visited every P-th step only (chunk c at the steps s with
 * (c % P + c / P + s) % P == 0) and then takes its pending updates at once, in step order, each with its own step's
 * scalars: the same fp32 operations per element as P = 1, a P-th of the bytes.  The ID vectors a rating reads catch
 * up in the head kernel's registers (rows_m / rows_v are read for that, also on a gradients-only step: pass them
 * whenever updates may be pending), a named row's entry wave applies what is missing before its gradient update.
 *   sweep_base / sweep_all: as for r4r_mf_step (the caller keeps the base; it becomes adam_step after sweep_all = 1,
 *   P = 1 or r4r_transnet_rows_flush).  lr, betas, eps, weight_decay do not change while updates are pending;
 *   r4r_transnet_rows_flush (adam_step = the last completed step; same `ws` / shapes as the steps) before anything else
 *   reads or writes the tables or their moments (evaluation through r4r_transnet_step included).  The int at
 *   r4r_transnet_ws_offset(which = 5) is set if more than 8 updates were ever pending (a broken schedule).
 * The data-parallel update launches (r4r_mf_apply, r4r_transnet_rows_apply, r4r_idnet_rows_apply) run the same
 * schedule over the gathered entries -- the same (P, base, all) on every rank. */
int r4r_transnet_rows_flush(const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                            int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes,
                            int64_t B, int T, int E, int L, int64_t V,
                            int sweep_period, int64_t sweep_base,
                            float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                            void *stream);

/* Data parallel: call r4r_transnet_step with flat_m == NULL (gradients only: flat_g and, TransNet++,
 * the compact ID-vector rows at r4r_transnet_ws_offset 1 / 2), exchange -- all-reduce flat_g and apply
 * r4r_adam_multi; all_gather the ranks' (uid, iid, gradient rows), ids -1 padding ragged shards --
 * then update the ID-vector tables from ALL ranks' rows (same `ws` and shape arguments as the step:
 * the row tags live there).  B_all <= 32768.  sweep_period / sweep_base / sweep_all: the schedule of the sweep, the
 * same on every rank (contract above; r4r_transnet_rows_flush on every rank). */
int r4r_transnet_rows_apply(const int64_t *uid_all, const int64_t *iid_all, const float *gu_all, const float *gi_all,
                            int sweep_period, int64_t sweep_base, int sweep_all,
                            int64_t B_all, const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                            int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes,
                            int64_t B, int T, int E, int L, int64_t V,
                            float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                            void *stream);
/* The same update with one exchange and no glue launches (world * B_pad <= 2,048 gathered ratings):
 * r4r_transnet_dp_block packs this rank's entries of the LAST gradients-only r4r_transnet_step on (uid, iid, ws)
 *   into `block` (r4r_transnet_dp_block_bytes(B_pad) bytes: ids as int32 + the two gradient rows; entries past B carry
 *   id -1), the caller all_gathers the blocks (rank order) and every rank calls
 * r4r_transnet_rows_apply_blocks(blocks [world], ...): the scheduled sweep straight over the blocks, ONE launch. */
size_t r4r_transnet_dp_block_bytes(int64_t B_pad);
int r4r_transnet_dp_block(const int64_t *uid, const int64_t *iid, void *ws, size_t ws_bytes, int64_t B, int T,
                          int E, int L, int64_t V, int64_t n_users, int64_t n_items, void *block, int64_t B_pad,
                          void *stream);
int r4r_transnet_rows_apply_blocks(const void *blocks, int world, int64_t B_pad, int sweep_period, int64_t sweep_base,
                                   int sweep_all, const uint64_t *rows_p, const uint64_t *rows_m,
                                   const uint64_t *rows_v, int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes,
                                   int64_t B, int T, int E, int L, int64_t V,
                                   float lr, double beta1, double beta2, float eps, float weight_decay,
                                   int64_t adam_step, void *stream);

/* ------------------------------------------------------------------------
 * Fused native step for the ID-only recommenders with dense layers: model_type 'MF' (MF.py:60-68) and
 * the NeuMF family (NeuMF.py: GMF :10-36, MLP :38-72, NeuMF :74-143; main.py:289-340 trains them in
 * three stages).  Replaces, per training step, the model's forward, MSELoss (loss.py:7-11),
 * loss.backward() and torch.optim.Adam.step() (main.py:56-60,94-96) by 3 launches (4 for NeuMF): a head
 * kernel per rating (forward + backward, compact ID-table gradient rows), the dense-gradient column sums
 * + Adam, and the tagged Adam sweeps over the ID tables and bias vectors (every row moves every step;
 * no dense table gradient is materialised).
 *   variant    0 MF   1 GMF   2 MLP   3 NeuMF
 *   flat_*     the dense parameters in r4r_idnet_layout order (8 slots; absent ones have size 0):
 *              projection/project .1.weight [L,2L], .1.bias, .3.weight [L,L], .3.bias, final.V [2L,L]
 *              (MF), final.lin.weight | final.weight [1, 2L or L], its bias, global_bias
 *   rows_*     HOST arrays of 6 device pointers: user / item table of the first pair (MF, GMF, MLP:
 *              user_embedding, item_embedding; NeuMF: gmf_*), of the second pair (NeuMF: mlp_*; else
 *              unused), user_bias, item_bias -- parameters, and their Adam moments
 *   flat_g == NULL: eval-mode forward only.  L <= 32, B <= 16384 for training steps. */
int r4r_idnet_nparam(void);
int r4r_idnet_layout(int variant, int L, int64_t *offsets, int64_t *sizes, int64_t *total);
size_t r4r_idnet_ws_bytes(int variant, int64_t B, int L, int64_t n_users, int64_t n_items);
size_t r4r_idnet_ws_offset(int variant, int64_t B, int L, int64_t n_users, int64_t n_items,
                           int which);   /* 0 dropout multipliers [B, draws], 1 d loss/d pred [B], 2 size of the persistent head (row tags), 3 the broken-schedule flag (int), 4 + 2*pair + side: compact gradient rows [B, L] */
int r4r_idnet_step(int variant, const int64_t *uid, const int64_t *iid, const float *y,
                   float *flat_p, float *flat_g, float *flat_m, float *flat_v,
                   const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                   int64_t n_users, int64_t n_items,
                   float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes,
                   int64_t B, int L, float dropout_p, int training, uint64_t seed, uint64_t offset,
                   float inv_denom, int sweep_period, int64_t sweep_base, int sweep_all,
                   float lr, double beta1, double beta2, float eps, float weight_decay,
                   int64_t adam_step, void *stream);
/* sweep_period / sweep_base / sweep_all: the sweeps over the variant's table pair(s), temporally blocked on the
 * schedule of r4r_mf_step (contract there and at r4r_transnet_rows_flush; rows_m / rows_v are read by the head kernel
 * for the catch-up of the rows a rating names, also on a gradients-only step; r4r_idnet_ws_offset which = 3: the
 * broken-schedule flag).  r4r_idnet_rows_flush applies what is pending; adam_step = the last completed step. */
int r4r_idnet_rows_flush(int variant, const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                         int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes, int64_t B, int L,
                         int sweep_period, int64_t sweep_base,
                         float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                         void *stream);

/* Data parallel: r4r_idnet_step with flat_m == NULL computes gradients only (flat_g, and in the workspace
 * d loss/d pred [B] and the compact rows [B, L] per table: r4r_idnet_ws_offset 1, 4..7); after the exchange --
 * all-reduce flat_g + r4r_adam_multi; all_gather of (uid, iid, d loss/d pred, rows), ids -1 padding ragged
 * shards -- the ID tables and bias vectors are updated from ALL ranks' rows.  gu_all / gi_all: HOST arrays of
 * 2 device pointers ([B_all, L] rows of the first / second table pair).  `ws`, B: the step's own.  B_all <= 16384.
 * sweep_period / sweep_base / sweep_all: as for r4r_transnet_rows_apply. */
int r4r_idnet_rows_apply(int variant, const int64_t *uid_all, const int64_t *iid_all, const float *g_all,
                         const uint64_t *gu_all, const uint64_t *gi_all,
                         int sweep_period, int64_t sweep_base, int sweep_all,
                         int64_t B_all,
                         const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                         int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes, int64_t B, int L,
                         float lr, double beta1, double beta2, float eps, float weight_decay,
                         int64_t adam_step, void *stream);

/* ------------------------------------------------------------------------
 * Device-side batch construction (the loader side of the path).
 * Replaces  data.DataLoader.remove_overlap / pad_and_join / pad_only and the 10-wide neighbour
 *           padding                                   data.py:144-236, 273-279, 375-447
 *           the per-batch LongTensor constructions    data.py:293-301, data_fast.py:101-109
 * The reviews of a dataset live in HBM as token pools (one per side; reviews4rec_amd/data.py):
 *   tok [tokens] int32, rev_off [reviews + 1] token range of a review, first [owners + 1] review
 *   range of a user / item, nb [reviews] the item / user a review is about (u_to_i_map / i_to_u_map)
 *   held_tok / held_off: the held-out reviews (test_reviews) as a pool of single reviews
 * For n ratings -- u, i: ids; nb_item: the item whose reviewer list is reported (== i except in
 * iter_negs, data.py:398); ku / ki: index of the rating's own review among the user's / item's
 * reviews, or -1 (nothing removed); held: index into the held pool or -1 ([0], data.py:245); train:
 * 1 = the own review is the user's review ku (data.py:221) -- ONE launch writes, as one int64 block,
 *   [n, doc] own review | [n, 10] users who reviewed the item (pad_user) | [n, 10] items the user
 *   reviewed (pad_item) | [n, doc] user document | [n, doc] item document
 * with doc = T (documents: reviews concatenated, cut / zero padded, R == 0) or R * W (NARRE: R
 * reviews of W words). */
int r4r_batch_build(const int32_t *user_tok, const int64_t *user_rev_off, const int64_t *user_first,
                    const int64_t *user_nb, const int32_t *item_tok, const int64_t *item_rev_off,
                    const int64_t *item_first, const int64_t *item_nb, const int32_t *held_tok,
                    const int64_t *held_off, const int64_t *u, const int64_t *i, const int64_t *nb_item,
                    const int64_t *ku, const int64_t *ki, const int64_t *held, int train, int64_t *out,
                    int64_t n, int T, int R, int W, int64_t pad_user, int64_t pad_item, void *stream);

/* ------------------------------------------------------------------------
 * Spans: K training steps per host call (csrc/span.hip).
 * Replaces  the body of the epoch loop, K iterations at a time        main.py:23-60
 *             for data, y in reader.iter(): zero_grad -> model(data) -> loss -> backward -> optimizer.step()
 *           with the batcher's slices                                  data_fast.py:99-109, data.py:250-372
 * for K consecutive FULL batches of an epoch: r4r_batch_build for a GROUP of batches per launch into a ring
 * of two groups, then the family's native step per batch, everything enqueued on `stream` from C.  The kernels are
 * those of the per-step entry points with the same arguments -- a span and K single steps give the same bits --; what
 * changes between two steps (batch pointers, adam_step, the dropout stream position, the token buffer, the sweep
 * schedule) advances here exactly as the per-step caller advances it.
 *
 * `loader`: HOST array of R4R_LOADER_WORDS uint64 describing the epoch (reviews4rec_amd/data.py builds it):
 *    0..3  user pool tok, rev_off, first, nb     4..7  item pool     8, 9  held_tok, held_off   (r4r_batch_build's)
 *   10..15 u, i, ku, ki, held (int64 [N]), y (float [N]): the epoch's ratings in loader order
 *   16 train  17 T  18 R  19 W  20 pad_user  21 pad_item                                          (r4r_batch_build's)
 *   22 ring: int64 device buffer of 2 groups, 0 = an ids-only loader (iter_simple: words 0..9, 12..14, 16..23 unused)
 *   23 ring stride per group (int64 elements, >= G * B * (3 doc + 20))   24 N   25 G batches per group   26 B
 *   27 0, or a HOST table [G][8] of the device pointers (r4r_span_batch's order) of G batches of B ratings that are
 *      already built and resident: batch b is entry b % G, nothing is constructed (a pool of batches cycled through;
 *      words 0..23 unused)
 * Batch b = ratings [b B, (b + 1) B); only the N / B full batches are reachable (a ragged tail goes through the
 * per-step entry).  built_group (host, in / out): the highest group whose block is in the ring, -1 before the
 * epoch's first span; groups are built in order as the steps reach them (the next one before the current one's last
 * step).  announce: a full batch follows the span and the last step announces it (its token marks ride on that
 * step's backward launch: pass tokens_ready = 1, token_buffer = the other buffer to whatever trains on it next).
 * steps_done (host, out, nullable): steps enqueued before an error.  token_buffer / tokens_ready / offset /
 * adam_step / sweep_*: the FIRST step's; step k runs with token_buffer ^ (k & 1), tokens_ready = 1 (k > 0),
 * offset + k * draws_per_step, adam_step + k.  sweep_period / sweep_want: the schedule in force and the one wanted
 * (engine.py _SweepSchedule: a step visits every chunk iff they differ or the period is 1, and the wanted one is in
 * force afterwards); *sweep_base / *sweep_period_out carry the schedule across calls.  Training steps only
 * (flat_g, moments and adam_step >= 1 required); all other arguments as in the family's r4r_*_step.  The documents a
 * span's steps read must be the ones the ring holds -- T = word 17 with R = word 18 = 0 (DeepCoNN, DeepCoNN++,
 * TransNet); NARRE: R, T = words 18, 19 and R = 10, the width of the neighbour lists -- and a resident table (word 27)
 * still takes NARRE's R = 10 only: anything else is refused before anything is enqueued (steps_done = 0).
 * r4r_span_build: make sure the group of `batch` is in the ring.  r4r_span_batch: the eight device pointers of a
 * built batch -- this, who, what, user doc, item doc, uid, iid, y (data_fast.py:101-109 order) -- into HOST slots[8]. */
#define R4R_LOADER_WORDS 28
int r4r_span_build(const uint64_t *loader, int64_t batch, int64_t *built_group, void *stream);
int r4r_span_batch(const uint64_t *loader, int64_t batch, uint64_t *slots);
int r4r_deepconn_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                      int64_t *built_group, int64_t *steps_done, const float *table, int64_t V, float *flat_p,
                      float *flat_g, float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes, int T,
                      int E, int L, float dropout_p, int training, uint64_t seed, uint64_t offset,
                      uint64_t draws_per_step, float inv_denom, int conv_algo, int token_buffer, int tokens_ready,
                      float *flat_m, float *flat_v, float lr, double beta1, double beta2, float eps,
                      float weight_decay, int64_t adam_step, void *stream);
/* Data parallel: r4r_deepconn_span with the gradient exchange between every step's gradients and its
 * Adam update -- step k = r4r_deepconn_step (gradients only, inv_denom = 1 / B_global) -> the collective -> the update,
 * everything enqueued from C.  exchange 0: `collective` = the address of RCCL's ncclAllReduce (in place on flat_g,
 * float32 sum), then r4r_adam_multi; exchange 1: ncclAllGather of flat_g into `gathered` [world][total], then
 * r4r_adam_gathered (rank order).  `collective` / `comm`: resolved and built by the caller in the RCCL library it
 * already holds (reviews4rec_amd/dist.py: StreamRccl); total = the flat layout's element count.  Replaces, per step,
 * the reference loop body of main.py:26-60 on every rank + the gradient sum the reference (single-process,
 * main.py:407) does not have. */
int r4r_deepconn_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                         int64_t *built_group, int64_t *steps_done, const float *table, int64_t V, float *flat_p,
                         float *flat_g, float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes, int T,
                         int E, int L, float dropout_p, int training, uint64_t seed, uint64_t offset,
                         uint64_t draws_per_step, float inv_denom, int conv_algo, int token_buffer, int tokens_ready,
                         float *flat_m, float *flat_v, int64_t total, float lr, double beta1, double beta2, float eps,
                         float weight_decay, int64_t adam_step, int exchange, void *collective, void *comm, int world,
                         float *gathered, void *stream);
int r4r_deepconnpp_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                        int64_t *built_group, int64_t *steps_done, const float *table, int64_t V, float *flat_p,
                        float *flat_g, float *flat_m, float *flat_v, const uint64_t *rows_p,
                        const uint64_t *rows_m, const uint64_t *rows_v, int64_t n_users, int64_t n_items,
                        float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes, int T, int E, int L,
                        float dropout_p, int training, uint64_t seed, uint64_t offset, uint64_t draws_per_step,
                        float inv_denom, int conv_algo, int token_buffer, int tokens_ready, float lr, double beta1,
                        double beta2, float eps, float weight_decay, int64_t adam_step, void *stream);
int r4r_narre_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce, int64_t *built_group,
                   int64_t *steps_done, const float *table, int64_t V, float *flat_p, float *flat_g, float *flat_m,
                   float *flat_v, const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v,
                   int64_t n_users, int64_t n_items, float *pred, float *se, float *sse_accum, void *ws,
                   size_t ws_bytes, int R, int T, int E, int L, float dropout_p, int training, uint64_t seed,
                   uint64_t offset, uint64_t draws_per_step, float inv_denom, int conv_algo, int token_buffer,
                   int tokens_ready, float lr, double beta1, double beta2, float eps, float weight_decay,
                   int64_t adam_step, void *stream);
int r4r_transnet_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                      int64_t *built_group, int64_t *steps_done, const float *table, int64_t V, float *flat_p,
                      float *flat_g, float *flat_m, float *flat_v, const uint64_t *rows_p, const uint64_t *rows_m,
                      const uint64_t *rows_v, int64_t n_users, int64_t n_items, float *pred, float *se,
                      float *sse_accum, void *ws, size_t ws_bytes, int T, int E, int L, int plus, float dropout_p,
                      int training, uint64_t seed, uint64_t offset, uint64_t draws_per_step, float inv_denom,
                      int conv_algo, int token_buffer, int tokens_ready, int sweep_period, int sweep_want,
                      int64_t *sweep_base, int *sweep_period_out, float lr, double beta1, double beta2, float eps,
                      float weight_decay, int64_t adam_step, void *stream);
int r4r_mf_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int64_t *steps_done, const uint64_t *p,
                const uint64_t *m, const uint64_t *v, int64_t n_users, int64_t n_items, int D, float *pred,
                float *se, float *sse_accum, void *ws, size_t ws_bytes, float dropout_p, int training,
                uint64_t seed, uint64_t offset, uint64_t draws_per_step, float inv_denom, int sweep_period,
                int sweep_want, int64_t *sweep_base, int *sweep_period_out, float lr, double beta1, double beta2,
                float eps, float weight_decay, int64_t adam_step, void *stream);
int r4r_idnet_span(const uint64_t *loader, int64_t first_batch, int64_t steps, int64_t *steps_done, int variant,
                   float *flat_p, float *flat_g, float *flat_m, float *flat_v, const uint64_t *rows_p,
                   const uint64_t *rows_m, const uint64_t *rows_v, int64_t n_users, int64_t n_items, float *pred,
                   float *se, float *sse_accum, void *ws, size_t ws_bytes, int L, float dropout_p, int training,
                   uint64_t seed, uint64_t offset, uint64_t draws_per_step, float inv_denom, int sweep_period,
                   int sweep_want, int64_t *sweep_base, int *sweep_period_out, float lr, double beta1,
                   double beta2, float eps, float weight_decay, int64_t adam_step, void *stream);
/* Data parallel for the other native families (csrc/span.hip): each r4r_<family>_span_dp enqueues, per step k, exactly
 * the launches, arguments, collectives and order of the engine's per-step data-parallel path (reviews4rec_amd/engine.py
 * _train_step_dp / _dp_rows) -- the family's step with gradients only (inv_denom = 1 / B_global), the collectives on
 * `stream`, the updates -- so an epoch through them leaves the bits of the per-step loop.  Replaces, per step, the
 * reference loop body of main.py:23-60 on every rank + the gradient exchange the reference (single-process) does not
 * have.  Arguments as in the family's span above, plus:
 *   total       the flat layout's element count (the all-reduce and r4r_adam_multi)
 *   allreduce / allgather   the addresses of RCCL's ncclAllReduce / ncclAllGather, resolved by the caller in the
 *               library it already holds (reviews4rec_amd/dist.py: StreamRccl), `comm` its communicator, `world` ranks;
 *               nothing is linked here.  The all-reduce is in place on flat_g (float32 sum); an all-gather moves
 *               `block` (this rank's bytes, as 4-byte words) into `blocks` [world] in rank order
 *   B_pad       every rank's shard is padded to it (hyper_params['batch_size']); the loader's B <= B_pad
 *   gathered    HOST array of the unpacked fields' device arrays [world * B_pad, width] (r4r_dp_unpack's dst)
 * Per step (adam_step + k):
 *   r4r_narre_span_dp       r4r_narre_step (flat / row moments NULL, sse on) -> ncclAllReduce(flat_g) ->
 *                           r4r_adam_multi -> r4r_narre_dp_block -> ncclAllGather(block -> blocks) ->
 *                           r4r_narre_rows_apply_blocks.  world * B_pad * (1 + R) <= 16384, L <= 32, R = 10.
 *                           (NARRE.py:18-19,110-116: the ID embeddings and biases whose rows travel)
 *   r4r_deepconnpp_span_dp  r4r_deepconnpp_step (gradients only) -> all-reduce -> r4r_adam_multi -> r4r_dp_pack (uid,
 *                           iid, d loss / d pred) -> all-gather -> r4r_dp_unpack into gathered[3] ->
 *                           r4r_deepconnpp_rows_apply.  world * B_pad <= 16384.  (DeepCoNN.py:64-72: the bias head)
 *   r4r_transnet_span_dp    r4r_transnet_step (gradients only, rows_m / rows_v read for the catch-up, on the sweep
 *                           schedule) -> all-reduce -> r4r_adam_multi -> TransNet++ only: r4r_transnet_dp_block ->
 *                           all-gather -> r4r_transnet_rows_apply_blocks; the schedule advances.  TransNet++:
 *                           world * B_pad <= 2048.  (TransNet.py:75-76,108-109: the ID vectors of TransNet++)
 *   r4r_idnet_span_dp       r4r_idnet_step (gradients only, on the schedule) -> all-reduce -> r4r_adam_multi ->
 *                           r4r_dp_pack (uid, iid, d loss / d pred, the compact rows of the 2 / NeuMF 4 tables) ->
 *                           all-gather -> r4r_dp_unpack into gathered[5 / 7] -> r4r_idnet_rows_apply; the schedule
 *                           advances.  world * B_pad <= 16384.  (MF.py:21-22,52-53 and NeuMF.py's embeddings)
 *   r4r_mf_span_dp          r4r_mf_grad (m / v / ws passed when rows may be pending: MF_dot on a schedule of period
 *                           > 1) -> ncclAllGather(block -> blocks) -> r4r_mf_apply (sse on); the schedule advances.
 *                           No all-reduce (allgather only); world * B_pad <= 16384; ws: r4r_mf_ws_bytes(world * B_pad).
 *                           (MF.py:21-22,52-53)
 * Every argument is checked before anything is enqueued (a refusal names the entry point, *steps_done = 0). */
int r4r_narre_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce, int64_t *built_group,
                      int64_t *steps_done, const float *table, int64_t V, float *flat_p, float *flat_g, float *flat_m,
                      float *flat_v, int64_t total, const uint64_t *rows_p, const uint64_t *rows_m,
                      const uint64_t *rows_v, int64_t n_users, int64_t n_items, float *pred, float *se,
                      float *sse_accum, void *ws, size_t ws_bytes, int R, int T, int E, int L, float dropout_p,
                      int training, uint64_t seed, uint64_t offset, uint64_t draws_per_step, float inv_denom,
                      int conv_algo, int token_buffer, int tokens_ready, float lr, double beta1, double beta2,
                      float eps, float weight_decay, int64_t adam_step, void *allreduce, void *allgather, void *comm,
                      int world, int64_t B_pad, void *block, void *blocks, void *stream);
int r4r_deepconnpp_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                           int64_t *built_group, int64_t *steps_done, const float *table, int64_t V, float *flat_p,
                           float *flat_g, float *flat_m, float *flat_v, int64_t total, const uint64_t *rows_p,
                           const uint64_t *rows_m, const uint64_t *rows_v, int64_t n_users, int64_t n_items,
                           float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes, int T, int E, int L,
                           float dropout_p, int training, uint64_t seed, uint64_t offset, uint64_t draws_per_step,
                           float inv_denom, int conv_algo, int token_buffer, int tokens_ready, float lr, double beta1,
                           double beta2, float eps, float weight_decay, int64_t adam_step, void *allreduce,
                           void *allgather, void *comm, int world, int64_t B_pad, void *block, void *blocks,
                           const uint64_t *gathered, void *stream);
int r4r_transnet_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int announce,
                         int64_t *built_group, int64_t *steps_done, const float *table, int64_t V, float *flat_p,
                         float *flat_g, float *flat_m, float *flat_v, int64_t total, const uint64_t *rows_p,
                         const uint64_t *rows_m, const uint64_t *rows_v, int64_t n_users, int64_t n_items,
                         float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes, int T, int E, int L,
                         int plus, float dropout_p, int training, uint64_t seed, uint64_t offset,
                         uint64_t draws_per_step, float inv_denom, int conv_algo, int token_buffer, int tokens_ready,
                         int sweep_period, int sweep_want, int64_t *sweep_base, int *sweep_period_out, float lr,
                         double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                         void *allreduce, void *allgather, void *comm, int world, int64_t B_pad, void *block,
                         void *blocks, void *stream);
int r4r_idnet_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int64_t *steps_done, int variant,
                      float *flat_p, float *flat_g, float *flat_m, float *flat_v, int64_t total,
                      const uint64_t *rows_p, const uint64_t *rows_m, const uint64_t *rows_v, int64_t n_users,
                      int64_t n_items, float *pred, float *se, float *sse_accum, void *ws, size_t ws_bytes, int L,
                      float dropout_p, int training, uint64_t seed, uint64_t offset, uint64_t draws_per_step,
                      float inv_denom, int sweep_period, int sweep_want, int64_t *sweep_base, int *sweep_period_out,
                      float lr, double beta1, double beta2, float eps, float weight_decay, int64_t adam_step,
                      void *allreduce, void *allgather, void *comm, int world, int64_t B_pad, void *block,
                      void *blocks, const uint64_t *gathered, void *stream);
int r4r_mf_span_dp(const uint64_t *loader, int64_t first_batch, int64_t steps, int64_t *steps_done, const uint64_t *p,
                   const uint64_t *m, const uint64_t *v, int64_t n_users, int64_t n_items, int D, float *pred,
                   float *se, float *sse_accum, void *ws, size_t ws_bytes, float dropout_p, int training,
                   uint64_t seed, uint64_t offset, uint64_t draws_per_step, float inv_denom, int sweep_period,
                   int sweep_want, int64_t *sweep_base, int *sweep_period_out, float lr, double beta1, double beta2,
                   float eps, float weight_decay, int64_t adam_step, void *allgather, void *comm, int world,
                   int64_t B_pad, void *block, void *blocks, void *stream);

/* ------------------------------------------------------------------------
 * Scoring spans: the forward-only launches of a validation / test / ranking pass, many per host call (csrc/span.hip).
 * Replaces  the loop of evaluate()          eval.py:24-40   for data, y in reader.iter(eval=True): model(data), criterion
 *           the loop of eval_ranking()      eval.py:64-78   for data, y in reader.iter_negs(): model(data)
 *           iter_negs' per-slice id lists   data.py:375-447 (six candidates per ranking row, the POSITIVE item's
 *                                                            overlap indices and reviewer list for all six)
 *           the batcher's slices            data_fast.py:99-109
 * `loader`: the R4R_LOADER_WORDS words of "Spans" above, every word with its meaning; n = word 26 is the LAUNCH size
 * (ratings scored per step, any size the caller's ring was made for -- not necessarily the training batch), and for
 * scoring only word 15 (y) may be 0: pure prediction, nothing is written to se_out.  Ranking rows are a descriptor
 * over the flattened candidates (N = 6 x rows, n a multiple of 6, word 15 = 0); `nb_item` (int64 [N], nullable) is
 * r4r_batch_build's: the item whose reviewer list is reported (data.py:398: the row's positive), NULL = i.
 * Launch k scores ratings [(first_launch + k) n, + n): its group (and the next launch's) is brought into the ring as a
 * training span does, then the family's own r4r_*_step runs in the form a per-launch caller's eval forward passes --
 * no gradients, no moments, training 0, tokens_ready 0, no next batch, inv_denom 1, adam_step 0, y = the slice of
 * word 15 or NULL -- with pred / se = pred_out + k n / se_out + k n of split-sized device arrays: the same kernels
 * with the same arguments, so every score keeps its bits.  token_buffer: launch 0's; launch k uses token_buffer ^
 * (k & 1) (DeepCoNN: only if token_alternate, else the same buffer every launch -- the other one holds an announced
 * batch).  DeepCoNN's sse_accum (nullable) += the sum of every launch's se, as its r4r_deepconn_step does.
 * TransNet(++): after each launch with ratings the per-rating (target SE, transform distance) pair -- columns 1:3 of
 * the workspace's [n, 3] (r4r_transnet_ws_offset which = 3) -- is copied to aux_out + k n 2; the other families
 * ignore aux_out.  Only the N / n full launches are reachable (a ragged tail goes through the per-step entry).
 * Refused before anything is enqueued (launches_done = 0): a launch range beyond N / n, NARRE with R != 10, a
 * resident table (word 27) together with nb_item, documents that are not the ring's, se_out NULL while word 15 is
 * set, aux_out NULL on TransNet.  The training entries above keep refusing a descriptor without y.
 *
 * r4r_rank_top1: HR@1's count (eval.py:79-88) over finished scores [rows, C] fp32, column 0 the positive, 2 <= C <=
 * 64.  counts (int64 [2], device) -- counts[0] += rows whose positive is STRICTLY greater than every other column;
 * counts[1] += rows that are UNDECIDED: the positive equals the maximum of the others, or the row holds a NaN (how
 * torch.topk orders those is the host's to decide).  Integer atomics only: the result does not depend on order. */
int r4r_rank_top1(const float *scores, int64_t rows, int C, int64_t *counts, void *stream);
int r4r_deepconn_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch, int64_t launches,
                            int64_t *built_group, int64_t *launches_done, const float *table, int64_t V,
                            float *flat_p, float *sse_accum, void *ws, size_t ws_bytes, int T, int E, int L,
                            float dropout_p, uint64_t seed, uint64_t offset, int conv_algo, int token_buffer,
                            int token_alternate, float *pred_out, float *se_out, float *aux_out, void *stream);
int r4r_deepconnpp_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch, int64_t launches,
                              int64_t *built_group, int64_t *launches_done, const float *table, int64_t V,
                              float *flat_p, const uint64_t *rows_p, int64_t n_users, int64_t n_items, void *ws,
                              size_t ws_bytes, int T, int E, int L, float dropout_p, uint64_t seed, uint64_t offset,
                              int conv_algo, int token_buffer, float *pred_out, float *se_out, float *aux_out,
                              void *stream);
int r4r_narre_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch, int64_t launches,
                         int64_t *built_group, int64_t *launches_done, const float *table, int64_t V, float *flat_p,
                         const uint64_t *rows_p, int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes, int R,
                         int T, int E, int L, float dropout_p, uint64_t seed, uint64_t offset, int conv_algo,
                         int token_buffer, float *pred_out, float *se_out, float *aux_out, void *stream);
int r4r_transnet_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch, int64_t launches,
                            int64_t *built_group, int64_t *launches_done, const float *table, int64_t V,
                            float *flat_p, const uint64_t *rows_p, int64_t n_users, int64_t n_items, void *ws,
                            size_t ws_bytes, int T, int E, int L, int plus, float dropout_p, uint64_t seed,
                            uint64_t offset, int conv_algo, int token_buffer, float *pred_out, float *se_out,
                            float *aux_out, void *stream);
int r4r_mf_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch, int64_t launches,
                      int64_t *built_group, int64_t *launches_done, const uint64_t *p, int64_t n_users,
                      int64_t n_items, int D, void *ws, size_t ws_bytes, float dropout_p, uint64_t seed,
                      uint64_t offset, float *pred_out, float *se_out, float *aux_out, void *stream);
int r4r_idnet_span_score(const uint64_t *loader, const int64_t *nb_item, int64_t first_launch, int64_t launches,
                         int64_t *built_group, int64_t *launches_done, int variant, float *flat_p,
                         const uint64_t *rows_p, int64_t n_users, int64_t n_items, void *ws, size_t ws_bytes, int L,
                         float dropout_p, uint64_t seed, uint64_t offset, float *pred_out, float *se_out,
                         float *aux_out, void *stream);

/* ------------------------------------------------------------------------
 * Catalogue recommendation: the K best candidates of each query row.
 * The reference has no such call: its ranking metric scores one positive against five sampled negatives, one forward
 * per pair (eval.py:76).  Three of its models score a pair as a dot product of a per-user and a per-item vector plus a
 * per-user and a per-item scalar, so a whole catalogue is ranked without a forward per pair:
 *   MF_dot     MF.py:56-58     vectors = the embedding tables in place, scalars = the bias tables (+ global bias)
 *   bias_only  MF.py:48-49     D = 0
 *   deepconn   DeepCoNN.py:61-66 over the FM of common_pytorch_models.py:49-57: with cat = [a | c], V = [Vu ; Vi],
 *              lin.weight = [wu | wi]:  fm(cat) = sum_f p_f q_f + [1/2 (sum_f p_f^2 - a^2 . Vu^2) + wu . a + lin.bias]
 *              + [1/2 (sum_f q_f^2 - c^2 . Vi^2) + wi . c],  p = a Vu, q = c Vi  (rank 8)
 *
 * score(u, i) is ONE fixed fp32 expression:  dot = fmaf(q[u][j], c[i][j], dot) for j = 0 .. D-1 ascending from +0.0f,
 * then (dot + c_bias[i]) + q_bias[u]; a NULL bias counts as 0.  v_mfma_f32_16x16x4_f32 computes exactly this chain,
 * zero-padding D to a multiple of 4 changes no bit, and D = 0 is a pure bias ranking.
 * Order: score descending, ties by ascending candidate id (a total order).  A candidate whose score is -inf or NaN
 * is never returned (-inf in c_bias marks a row ineligible), nor one listed in the query's exclusion list; when fewer
 * than K remain, the unused slots hold id -1 and score -inf.
 * The result depends on the inputs only: not on `chunk`, the grid, or which other queries share the call -- query u
 * answered alone and inside a batch gives the same ids and the same score bits.
 *   q [n_q, D] dense, q_bias [n_q] or NULL;  c rows c_stride >= D floats apart, c_bias [n_c] or NULL
 *   excl_off [n_q + 1], excl_ids: CSR per query row, ids strictly ascending; both NULL = no exclusions
 *   chunk: candidates per partial list, 0 = the library's choice;  out_ids / out_scores [n_q, K]
 * Limits: 0 <= D <= 256 (MF_dot's native limit), 1 <= K <= 128, n_q, n_c >= 0; n_q == 0 or n_c == 0 returns R4R_OK
 * and enqueues nothing (the outputs are not touched).  Every refusal precedes the first launch; a short workspace is
 * R4R_ERR_WORKSPACE.  Two launches (scan, merge), or one when the catalogue is a single chunk.
 *
 * r4r_pair_dot: the same expression for n explicit pairs (q_idx[p], c_idx[p]) -> out[p].
 *
 * r4r_rank_dot: the rank of explicit targets in that order, the count full-catalogue HR@K / NDCG@K / MRR are made of.
 * It generalises the reference's only ranking call site, eval.py:64-92 (one positive against five sampled negatives),
 * to the positive against every candidate.  Pair p = (query row q_idx[p], target candidate t_idx[p]); several pairs may
 * share a query row and a pair may appear twice.
 *   out_score[p] = score(q_idx[p], t_idx[p]), the bits of r4r_pair_dot
 *   out_rank[p]  = the number of candidates j in [0, n_c) whose score is neither -inf nor NaN, that are not in the
 *                  exclusion list of query row q_idx[p], and that are AHEAD of the target t:
 *                  s_j > s_t || (s_j == s_t && j < t).  The target never counts against itself, excluded or not.
 *                  A target whose own score is -inf or NaN gets rank -1.
 *   excl_off [n_q + 1] is over query ROWS (not pairs), ids ascending; both NULL = no exclusions
 *   chunk: candidates per workgroup pass, 0 = the library's choice
 * The rank is an integer summed by integer atomics: the same for every `chunk`, every tiling and every grouping of the
 * pairs into calls.  Limits: 0 <= D <= 256, c_stride >= D, n_q, n_c, n_p >= 0, 0 <= chunk <= 2^30; q_idx / t_idx out
 * of range is the caller's error, as in r4r_pair_dot.  n_p == 0 or n_c == 0 returns R4R_OK and enqueues nothing (the
 * outputs are not touched).  Every refusal precedes the first launch.  No workspace.  Three launches: targets, the
 * fused MFMA scan with counters in place of lists, and -- only with exclusions -- a correction that recomputes the
 * excluded ids' scalar chains (exact: a score's bits depend on its own pair only).
 * ---------------------------------------------------------------------- */
size_t r4r_topk_dot_ws_bytes(int64_t n_q, int64_t n_c, int K, int64_t chunk);
int r4r_topk_dot(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                 const float *c_bias, int D, const int64_t *excl_off, const int64_t *excl_ids, int K, int64_t chunk,
                 void *ws, size_t ws_bytes, int64_t *out_ids, float *out_scores, void *stream);
int r4r_pair_dot(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                 const float *c_bias, int D, const int64_t *q_idx, const int64_t *c_idx, int64_t n, float *out,
                 void *stream);
int r4r_rank_dot(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                 const float *c_bias, int D, const int64_t *q_idx, const int64_t *t_idx, int64_t n_p,
                 const int64_t *excl_off, const int64_t *excl_ids, int64_t chunk, int64_t *out_rank, float *out_score,
                 void *stream);

/* ------------------------------------------------------------------------
 * Catalogue recommendation: ReLU-sum heads.  The same lists, pair scores and ranks for the models whose head is
 * Linear -> ReLU -> (linear down to one scalar) over [user | item].  The first Linear separates over the
 * concatenation, W [x_u ; x_i] + b = (W_u x_u + b) + W_i x_i, and everything after the ReLU is linear, so with per-user
 * rows q = [qa | qp], per-item rows c = [ca | cp] and one weight vector w:
 *   deepconn++  DeepCoNN.py:68-72    H = L, P = 0: qa = W0[:, :L] zu + b0, ca = W0[:, L:] zi, w = final.3.weight
 *   NeuMF       NeuMF.py:25-38       stage GMF: H = 0, P = L: qp = user_embedding * final.weight, cp = item_embedding
 *               NeuMF.py:60-74       stage MLP: H = L, P = 0: qa = W1[:, :L] ue + b1, ca = W1[:, L:] ie, w = f W3
 *               NeuMF.py:120-143     stage NeuMF: H = L, P = L: both of the above on the mlp_* / gmf_* tables
 * (the remaining scalars go to q_bias / c_bias; reviews4rec_amd.recommend.fold_relu_head has the table).
 *
 * score(u, i) is ONE fixed fp32 expression, both chains ascending in j from +0.0f:
 *   h = fmaf(w[j], fmaxf(q[u][j] + c[i][j], 0.f), h)        j = 0 .. H-1
 *   d = fmaf(q[u][H + j], c[i][H + j], d)                   j = 0 .. P-1
 *   score = ((h + d) + c_bias[i]) + q_bias[u]               a NULL bias counts as 0
 * fmaxf is C's: a NaN sum in a hidden column counts as 0 (mark a row ineligible through c_bias, not through NaN columns
 * of the hidden part).  With H = 0 this is r4r_topk_dot's expression at D = P, bit for bit.
 *   q [n_q, H + P] dense, q_bias [n_q] or NULL;  c rows c_stride >= H + P floats apart (the pad is never read),
 *   c_bias [n_c] or NULL;  w [H]
 * Everything else is r4r_topk_dot's contract: score descending, ties by ascending candidate id; a candidate whose score
 * is -inf or NaN is never returned (-inf in c_bias marks a row ineligible), nor one on the query's ascending CSR
 * exclusion list (excl_off [n_q + 1], excl_ids; both NULL = none); unused slots hold id -1 and score -inf.  The order
 * is total and a score's bits depend on its own pair only: the result does not depend on `chunk`, the grid, or how
 * queries and pairs are grouped into calls.
 * Limits: 0 <= H <= 128, 0 <= P <= 128, 1 <= K <= 128, 0 <= chunk <= 2^30 (0 = the library's choice), c_stride >= H + P,
 * w non-NULL when H > 0, q and c non-NULL when H + P > 0, excl_off and excl_ids both or neither.  n_q == 0, n_c == 0 or
 * n_p == 0 returns R4R_OK, enqueues nothing and leaves the outputs untouched.  Every refusal precedes the first launch
 * and the first dereference; a short workspace is R4R_ERR_WORKSPACE.  Nothing allocates, nothing synchronises.
 *
 * r4r_topk_relu: out_ids / out_scores [n_q, K].  Two launches (a VALU scan, lane = candidate; r4r_topk_dot's merge), or
 * one when the catalogue is a single chunk.  The workspace holds the chunks' partial lists in r4r_topk_dot's layout.
 * r4r_pair_relu: the same expression for n explicit pairs (q_idx[p], c_idx[p]) -> out[p].
 * r4r_rank_relu: r4r_rank_dot's semantics exactly -- the full-catalogue generalisation of eval.py:64-92.  out_score[p]
 *   has r4r_pair_relu's bits; out_rank[p] counts the candidates ahead of target t_idx[p] for query row q_idx[p] that
 *   are neither -inf / NaN nor on that ROW's exclusion list; the target never counts against itself; a target whose own
 *   score is -inf or NaN gets -1.  Integer atomics only: equal for every chunk, tiling and grouping.  No workspace.
 * ---------------------------------------------------------------------- */
size_t r4r_topk_relu_ws_bytes(int64_t n_q, int64_t n_c, int K, int64_t chunk);
int r4r_topk_relu(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                  const float *c_bias, const float *w, int H, int P, const int64_t *excl_off, const int64_t *excl_ids,
                  int K, int64_t chunk, void *ws, size_t ws_bytes, int64_t *out_ids, float *out_scores, void *stream);
int r4r_pair_relu(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                  const float *c_bias, const float *w, int H, int P, const int64_t *q_idx, const int64_t *c_idx,
                  int64_t n, float *out, void *stream);
int r4r_rank_relu(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                  const float *c_bias, const float *w, int H, int P, const int64_t *q_idx, const int64_t *t_idx,
                  int64_t n_p, const int64_t *excl_off, const int64_t *excl_ids, int64_t chunk, int64_t *out_rank,
                  float *out_score, void *stream);

/* ------------------------------------------------------------------------
 * Catalogue recommendation: product-MLP heads.  The same lists, pair scores and ranks for a model whose head is
 * Linear -> ReLU -> Linear over the ELEMENTWISE PRODUCT of a per-user and a per-item vector:
 *   NARRE   NARRE.py:38-43,121-124   final = Dropout, Linear(L, L), ReLU, Linear(L, 1) over (user + user_vec) * (item + item_vec)
 *           NARRE.py:53-64,110-119   the user-side attention reads the embeddings of the items the user's OWN reviews are
 *                                    about (reviewed_items), the item side those of the users who reviewed the item
 *                                    (users_who_reviewed): neither reads the other member of the pair
 *           data.py:240-246          for a rating outside the training split nothing is removed from either side
 * so both attended vectors are functions of one side only: q[u] = attention_user(u) + user_embedding[u], c[i] =
 * attention_item(i) + item_embedding[i], W = final.1.weight, b = final.1.bias, w = final.3.weight, and the remaining
 * scalars go to q_bias / c_bias (reviews4rec_amd.recommend.NarreCatalogue).
 *
 * score(u, i) is ONE fixed fp32 expression:
 *   x_m = q[u][m] * c[i][m]                                   one fp32 multiply, m = 0 .. D-1
 *   y_j = fmaf(W[j][m], x_m, y_j)                             m ascending from +0.0f, j = 0 .. H-1
 *   z_j = fmaxf(y_j + b[j], 0.f)                              C's fmaxf: a NaN sum counts as 0, as in r4r_topk_relu
 *   h_g = fmaf(w[j], z_j, h_g)                                over the j with ((j >> 2) & 3) == g, ascending from +0.0f, g = 0 .. 3
 *   score = ((((h_0 + h_1) + (h_2 + h_3)) + c_bias[i]) + q_bias[u])
 * The four-way split of the last sum is the accumulator layout of v_mfma_f32_16x16x4_f32 with rows = hidden units: lane
 * group l >> 4 holds rows 4 g + r of every 16, so the epilogue is four chains and two cross-lane adds.  A NULL b, q_bias
 * or c_bias counts as 0.  Zero-padding D to a multiple of 4 and H to a multiple of 16 changes no bit: a pad column
 * multiplies 0 by 0, a pad row of W gives z = 0, and the pad entries of b and w are zero.  (A NaN anywhere in a
 * candidate's row makes every y NaN, every z 0 and the score the sum of the biases: mark a row ineligible through c_bias.)
 *   q [n_q, D] dense, q_bias [n_q] or NULL;  c rows c_stride >= D floats apart (the pad is never read), c_bias [n_c] or
 *   NULL;  W [H, D] dense, row-major;  b [H] or NULL;  w [H]
 * Everything else is r4r_topk_dot's contract: score descending, ties by ascending candidate id; a candidate whose score
 * is -inf or NaN is never returned (-inf in c_bias marks a row ineligible), nor one on the query's ascending CSR
 * exclusion list (excl_off [n_q + 1], excl_ids; both NULL = none); unused slots hold id -1 and score -inf.  The order
 * is total and a score's bits depend on its own pair only: the result does not depend on `chunk`, the grid, or how
 * queries and pairs are grouped into calls.
 * Limits: 0 <= D <= 64, 0 <= H <= 64 (the native limit of NARRE's engine), 1 <= K <= 128, 0 <= chunk <= 2^30 (0 = the
 * library's choice), c_stride >= D, w and W non-NULL when H > 0, q and c non-NULL when D > 0, excl_off and excl_ids both
 * or neither.  n_q == 0, n_c == 0 or n_p == 0 returns R4R_OK, enqueues nothing and leaves the outputs untouched.  Every
 * refusal precedes the first launch and the first dereference; a short workspace is R4R_ERR_WORKSPACE.  Nothing
 * allocates, nothing synchronises.
 *
 * r4r_topk_hmlp: out_ids / out_scores [n_q, K].  Two launches (an MFMA scan whose A operand is W and whose B operand is
 *   q * c formed in registers; r4r_topk_dot's merge), or one when the catalogue is a single chunk.  The workspace holds
 *   the chunks' partial lists in r4r_topk_dot's layout.
 * r4r_pair_hmlp: the same expression for n explicit pairs (q_idx[p], c_idx[p]) -> out[p].
 * r4r_rank_hmlp: r4r_rank_dot's semantics exactly.  out_score[p] has r4r_pair_hmlp's bits; out_rank[p] counts the
 *   candidates ahead of target t_idx[p] for query row q_idx[p] that are neither -inf / NaN nor on that ROW's exclusion
 *   list; the target never counts against itself; a target whose own score is -inf or NaN gets -1.  Integer atomics
 *   only: equal for every chunk, tiling and grouping.  No workspace.
 * ---------------------------------------------------------------------- */
size_t r4r_topk_hmlp_ws_bytes(int64_t n_q, int64_t n_c, int K, int64_t chunk);
int r4r_topk_hmlp(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                  const float *c_bias, const float *W, const float *b, const float *w, int D, int H,
                  const int64_t *excl_off, const int64_t *excl_ids, int K, int64_t chunk, void *ws, size_t ws_bytes,
                  int64_t *out_ids, float *out_scores, void *stream);
int r4r_pair_hmlp(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                  const float *c_bias, const float *W, const float *b, const float *w, int D, int H,
                  const int64_t *q_idx, const int64_t *c_idx, int64_t n, float *out, void *stream);
int r4r_rank_hmlp(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                  const float *c_bias, const float *W, const float *b, const float *w, int D, int H,
                  const int64_t *q_idx, const int64_t *t_idx, int64_t n_p, const int64_t *excl_off,
                  const int64_t *excl_ids, int64_t chunk, int64_t *out_rank, float *out_score, void *stream);

/* ------------------------------------------------------------------------
 * Catalogue recommendation: ReLU-FM heads.  The same lists, pair scores and ranks for a model whose head is
 * Linear -> ReLU -> Linear -> FM over [user | item]:
 *   TransNet(++)  TransNet.py:14-35      the source network: two towers over one side's document each, project =
 *                                        Linear(2 L, L), ReLU, Linear(L, L) over [user tower | item tower]
 *                 TransNet.py:105-119    the test-time score: source_fm over the source network's output (transnet++:
 *                                        over [user_embedding | item_embedding | output]), column 0; it reads no
 *                                        review of the pair
 *                 common_pytorch_models.py:41-57   the FM: lin(x) + 1/2 sum_f ((x V)_f^2 - (x^2 V^2)_f)
 *                 data.py:240-246        for a rating outside the training split nothing is removed from either document
 *                 eval.py:31-32          the score is output[0] (eval.py:72 for the ranking metric)
 * The first Linear separates, W0 [zu ; zi] + b0 = (W0[:, :L] zu + b0) + W0[:, L:] zi, and an FM of a linear image of
 * h = relu(.) is a short sum of signed squares and one linear term of y = W h + b: rows (W2^T Vr)^T with s = +1/2, rows
 * diag(sqrt(sum_f Vr^2)) W2 with s = -1/2, and one row lr^T W2 with l = 1 (reviews4rec_amd.recommend.fold_transnet_head
 * has the table; transnet++'s embedding terms enter as P = 8 plain input columns and two scalars).
 *
 * score(u, i) is ONE fixed fp32 expression, D = H + P:
 *   x_m = fmaxf(q[u][m] + c[i][m], 0.f)   m < H               C's fmaxf: a NaN sum counts as 0
 *   x_m = q[u][m] + c[i][m]               H <= m < D          plain: a NaN here reaches the score
 *   y_j = fmaf(W[j][m], x_m, y_j)                             m ascending from +0.0f, then y_j = y_j + b[j], j = 0 .. M-1
 *   e_j = fmaf(s[j], y_j, l[j])
 *   t_g = fmaf(e_j, y_j, t_g)                                 over the j with ((j >> 2) & 3) == g, ascending from +0.0f, g = 0 .. 3
 *   score = ((((t_0 + t_1) + (t_2 + t_3)) + c_bias[i]) + q_bias[u])
 * The four-way split of the last sum is the accumulator layout of v_mfma_f32_16x16x4_f32 with rows = rows of y: lane
 * group l >> 4 holds rows 4 g + r of every 16, so the epilogue is four chains and two cross-lane adds.  A NULL b, q_bias
 * or c_bias counts as 0.  Zero-padding D to a multiple of 4 and M to a multiple of 16 changes no bit: a pad column
 * multiplies by W = 0, and a pad row (W, b, s, l all zero) gives y = 0, e = 0 and adds e y = 0 to its chain.
 *   q [n_q, D] dense, q_bias [n_q] or NULL;  c rows c_stride >= D floats apart (the pad is never read), c_bias [n_c] or
 *   NULL;  W [M, D] dense, row-major;  b [M] or NULL;  s [M], l [M]
 * Everything else is r4r_topk_dot's contract: score descending, ties by ascending candidate id; a candidate whose score
 * is -inf or NaN is never returned (-inf in c_bias marks a row ineligible), nor one on the query's ascending CSR
 * exclusion list (excl_off [n_q + 1], excl_ids; both NULL = none); unused slots hold id -1 and score -inf.  The order
 * is total and a score's bits depend on its own pair only: the result does not depend on `chunk`, the grid, or how
 * queries and pairs are grouped into calls.
 * Limits: 0 <= H <= 64 (the native limit of the TransNet engine), 0 <= P <= 16, 0 <= M <= 80, 1 <= K <= 128,
 * 0 <= chunk <= 2^30 (0 = the library's choice), c_stride >= D, W, s and l non-NULL when M > 0, q and c non-NULL when
 * D > 0, excl_off and excl_ids both or neither.  n_q == 0, n_c == 0 or n_p == 0 returns R4R_OK, enqueues nothing and
 * leaves the outputs untouched.  Every refusal precedes the first launch and the first dereference; a short workspace
 * is R4R_ERR_WORKSPACE.  Nothing allocates, nothing synchronises.
 *
 * r4r_topk_rfm: out_ids / out_scores [n_q, K].  Two launches (an MFMA scan whose A operand is W and whose B operand is
 *   relu(q + c) formed in registers; r4r_topk_dot's merge), or one when the catalogue is a single chunk.  The workspace
 *   holds the chunks' partial lists in r4r_topk_dot's layout.
 * r4r_pair_rfm: the same expression for n explicit pairs (q_idx[p], c_idx[p]) -> out[p].
 * r4r_rank_rfm: r4r_rank_dot's semantics exactly.  out_score[p] has r4r_pair_rfm's bits; out_rank[p] counts the
 *   candidates ahead of target t_idx[p] for query row q_idx[p] that are neither -inf / NaN nor on that ROW's exclusion
 *   list; the target never counts against itself; a target whose own score is -inf or NaN gets -1.  Integer atomics
 *   only: equal for every chunk, tiling and grouping.  No workspace.
 * ---------------------------------------------------------------------- */
size_t r4r_topk_rfm_ws_bytes(int64_t n_q, int64_t n_c, int K, int64_t chunk);
int r4r_topk_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                 const float *c_bias, const float *W, const float *b, const float *s, const float *l, int H, int P, int M,
                 const int64_t *excl_off, const int64_t *excl_ids, int K, int64_t chunk, void *ws, size_t ws_bytes,
                 int64_t *out_ids, float *out_scores, void *stream);
int r4r_pair_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                 const float *c_bias, const float *W, const float *b, const float *s, const float *l, int H, int P, int M,
                 const int64_t *q_idx, const int64_t *c_idx, int64_t n, float *out, void *stream);
int r4r_rank_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                 const float *c_bias, const float *W, const float *b, const float *s, const float *l, int H, int P, int M,
                 const int64_t *q_idx, const int64_t *t_idx, int64_t n_p, const int64_t *excl_off,
                 const int64_t *excl_ids, int64_t chunk, int64_t *out_rank, float *out_score, void *stream);

/* ------------------------------------------------------------------------
 * Catalogue recommendation: product-FM heads.  The same lists, pair scores and ranks for a model whose head is an FM
 * over [Linear -> ReLU -> Linear of [user | item]  |  user * item]:
 *   MF            MF.py:45-49 / 60-66    projection = Linear(2 L, L), ReLU, Linear(L, L) over [user embedding | item
 *                                        embedding]; final = FM(2 L, L) over [projection | user embedding * item embedding]
 *                 common_pytorch_models.py:41-57   the FM: lin(x) + 1/2 sum_f ((x V)_f^2 - (x^2 V^2)_f)
 * The first Linear separates, W1 [ue ; ie] + b1 = (W1[:, :L] ue + b1) + W1[:, L:] ie; with h = relu(.) and m = ue * ie the
 * FM's input is [W3 h + b3 ; m], so its squares are signed squares of y = W [h ; m] + b (rows (W3^T Va | Vb^T) with
 * s = +1/2, rows diag(sqrt(sum_f Va^2)) W3 with s = -1/2), and everything else is PER COLUMN of x = [h ; m]: the linear
 * term e = [la^T W3 | lm], and -1/2 sigma_b m^2 as g x^2 -- the square of a product column is that column's own x^2
 * (reviews4rec_amd.recommend.fold_mf_head has the table).
 *
 * score(u, i) is ONE fixed fp32 expression, D = H + G:
 *   x_m = fmaxf(q[u][m] + c[i][m], 0.f)   m < H               C's fmaxf: a NaN sum counts as 0
 *   x_m = q[u][m] * c[i][m]               H <= m < D          a product: a NaN here reaches the score
 *   y_j = fmaf(W[j][m], x_m, y_j)                             m ascending from +0.0f, then y_j = y_j + b[j], j = 0 .. M-1
 *   t_k = fmaf(s[j] * y_j, y_j, t_k)                          over the j with ((j >> 2) & 3) == k, ascending from +0.0f
 *   v_k = fmaf(fmaf(g[m], x_m, e[m]), x_m, v_k)               over the m with (m & 3) == k, ascending from +0.0f, k = 0 .. 3
 *   score = (((((t_0 + v_0) + (t_1 + v_1)) + ((t_2 + v_2) + (t_3 + v_3))) + c_bias[i]) + q_bias[u])
 * (s[j] * y_j is one rounded product.)  The four-way split of both sums is the layout of v_mfma_f32_16x16x4_f32 with
 * rows = rows of y: lane group l >> 4 holds rows 4 k + r of every 16 of the result and columns 4 t + k of the input it
 * forms, so the epilogue is four row chains, the four column chains the same lanes carried along, one add of the two
 * and two cross-lane adds; the scalar pair kernel writes the same chain out and gives the scan's bits.  A NULL b, g, e,
 * q_bias or c_bias counts as 0.  Zero-padding D to a multiple of 4 and M to a multiple of 16 changes no bit: a pad
 * column (q = c = 0, so x = 0; W, g, e zero) adds fmaf(fmaf(0, 0, 0), 0, v_k) = v_k and multiplies by W = 0, and a pad
 * row (W, b, s zero) gives y = 0 and adds fmaf(0, 0, t_k) = t_k.
 *   q [n_q, D] dense, q_bias [n_q] or NULL;  c rows c_stride >= D floats apart (the pad is never read), c_bias [n_c] or
 *   NULL;  W [M, D] dense, row-major;  b [M] or NULL;  s [M];  g [D] or NULL;  e [D] or NULL
 * Everything else is r4r_topk_dot's contract: score descending, ties by ascending candidate id; a candidate whose score
 * is -inf or NaN is never returned (-inf in c_bias marks a row ineligible), nor one on the query's ascending CSR
 * exclusion list (excl_off [n_q + 1], excl_ids; both NULL = none); unused slots hold id -1 and score -inf.  The order
 * is total and a score's bits depend on its own pair only: the result does not depend on `chunk`, the grid, or how
 * queries and pairs are grouped into calls.
 * Limits: 0 <= H <= 64, 0 <= G <= 64, 0 <= M <= 128, 1 <= K <= 128, 0 <= chunk <= 2^30 (0 = the library's choice),
 * c_stride >= D, W and s non-NULL when M > 0, q and c non-NULL when D > 0, excl_off and excl_ids both or neither.
 * n_q == 0, n_c == 0 or n_p == 0 returns R4R_OK, enqueues nothing and leaves the outputs untouched.  Every refusal
 * precedes the first launch and the first dereference; a short workspace is R4R_ERR_WORKSPACE.  Nothing allocates,
 * nothing synchronises.  The head lives in LDS (W in MFMA fragment order, shared by the four waves of a workgroup); above
 * 64 x 64 a scan needs more than 64 KiB of it, and each of the three calls raises that kernel's limit (once per
 * device) before its FIRST launch -- where the runtime refuses that, the call returns R4R_ERR_LAUNCH, has launched
 * nothing and has written no output.
 *
 * r4r_topk_pfm: out_ids / out_scores [n_q, K].  Two launches (an MFMA scan whose A operand is W, read from LDS, and whose
 *   B operand is formed in registers; r4r_topk_dot's merge), or one when the catalogue is a single chunk.  The workspace
 *   holds the chunks' partial lists in r4r_topk_dot's layout.
 * r4r_pair_pfm: the same expression for n explicit pairs (q_idx[p], c_idx[p]) -> out[p].
 * r4r_rank_pfm: r4r_rank_dot's semantics exactly.  out_score[p] has r4r_pair_pfm's bits; out_rank[p] counts the
 *   candidates ahead of target t_idx[p] for query row q_idx[p] that are neither -inf / NaN nor on that ROW's exclusion
 *   list; the target never counts against itself; a target whose own score is -inf or NaN gets -1.  Integer atomics
 *   only: equal for every chunk, tiling and grouping.  No workspace.
 * ---------------------------------------------------------------------- */
size_t r4r_topk_pfm_ws_bytes(int64_t n_q, int64_t n_c, int K, int64_t chunk);
int r4r_topk_pfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                 const float *c_bias, const float *W, const float *b, const float *s, const float *g, const float *e,
                 int H, int G, int M, const int64_t *excl_off, const int64_t *excl_ids, int K, int64_t chunk, void *ws,
                 size_t ws_bytes, int64_t *out_ids, float *out_scores, void *stream);
int r4r_pair_pfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                 const float *c_bias, const float *W, const float *b, const float *s, const float *g, const float *e,
                 int H, int G, int M, const int64_t *q_idx, const int64_t *c_idx, int64_t n, float *out, void *stream);
int r4r_rank_pfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                 const float *c_bias, const float *W, const float *b, const float *s, const float *g, const float *e,
                 int H, int G, int M, const int64_t *q_idx, const int64_t *t_idx, int64_t n_p, const int64_t *excl_off,
                 const int64_t *excl_ids, int64_t chunk, int64_t *out_rank, float *out_score, void *stream);

/* ------------------------------------------------------------------------
 * Tower spans: one side's catalogue towers from the resident pools, enqueued from C (csrc/tower_span.hip).
 * Replaces  the documents a rating outside the training split is scored with -- every review of the owner, nothing
 *           removed                                                     data.py:240-246
 *           pad_and_join / pad_only: cut / zero padded to input_length  data.py:181-210
 *           NARRE's [R, W] review layout                                data.py:144-172
 *           the 10-wide neighbour lists and their pad ids               data.py:275-279
 *           as the catalogue classes evaluate them on the host (reviews4rec_amd/recommend.py: Catalogue._documents,
 *           NarreCatalogue._attended -- numpy over the pools, one [n, T] int64 block copied per tower_batch owners), and
 *           the per-chunk Python call sites of Catalogue._tower (r4r_textcnn_fwd + r4r_linear_fwd) in refresh() /
 *           _queries() of Catalogue, ReluCatalogue, NarreCatalogue and TransNetCatalogue.
 * One side's pool (r4r_batch_build's layout): tok [tokens + 1] int32, rev_off [reviews + 1], first [owners + 1],
 * nb [reviews] (NULL for a pool without a single review: an empty array has no address; every neighbour is `pad` then);
 * ids [n] int64 owner ids ON THE DEVICE, in any order, repeats allowed.
 *
 * r4r_tower_build: ONE launch, nothing removed.  R == 0: docs [n, T] = every review of owner ids[r] concatenated, cut /
 *   zero padded to T; neigh is not written and may be NULL.  R > 0 (NARRE): docs [n, R, W], slot r = the r-th review cut
 *   / padded to W, and neigh [n, 10] = the nb entries of the first 10 reviews, missing ones `pad`.  Integer for integer
 *   what data._np_docs / _np_reviews / _np_neighbours return with skip = -1.  An id outside [0, owners) is an owner
 *   without reviews (a zero document, `pad` neighbours): nothing outside the pool is read whatever ids holds.
 *   n == 0 returns R4R_OK and enqueues nothing.  Shape rules: r4r_batch_build's (0 < n < 2^31; R > 0 and W > 0, or R == 0
 *   and T > 0), owners >= 0.
 *
 * r4r_tower_span_fwd: the tower over n owners, `group` owners per round.  Round g covers owners [g group, min(n, (g + 1)
 *   group)) and enqueues r4r_tower_build into the workspace, r4r_textcnn_fwd over the round's rows (owners x max(R, 1)
 *   rows of T or W words) and r4r_linear_fwd (no ReLU) into latent + g group max(R, 1) L.  latent [n, L], or [n R, L]
 *   with R > 0; neigh [n, 10] with R > 0, else NULL.  table [V, E], conv_w [F, 3, E], conv_b [F] as r4r_textcnn_fwd takes
 *   them (E % 4 == 0: a caller with another width pads the table and the weight), fc_w [L, F], fc_b [L].  The kernels and
 *   their arguments are those of the per-call entry points, and r4r_textcnn_fwd resolves its algorithm from the round's
 *   rows as it does per call: a span over `group` gives the bits of one r4r_textcnn_fwd + r4r_linear_fwd call per chunk
 *   of `group` owners.  ws: r4r_tower_span_ws_bytes(group, ...) bytes -- one round's documents, pooled values, argmax and
 *   r4r_textcnn_ws_bytes of a full round; stream order makes its reuse across rounds safe.  groups_done (host, out,
 *   nullable): rounds enqueued before an error.  Refused before the first launch, with r4r_last_error set: null
 *   pointers, group < 1, E % 4 != 0, F > 112, r4r_tower_build's shape rules, a short workspace (R4R_ERR_WORKSPACE).
 *   n == 0 returns R4R_OK and enqueues nothing.  Nothing allocates, nothing synchronises, no training state is touched.
 * ---------------------------------------------------------------------- */
int r4r_tower_build(const int32_t *tok, const int64_t *rev_off, const int64_t *first, const int64_t *nb,
                    int64_t owners, const int64_t *ids, int64_t n, int T, int R, int W, int64_t pad,
                    int64_t *docs, int64_t *neigh, void *stream);
size_t r4r_tower_span_ws_bytes(int64_t group, int T, int R, int W, int E, int F, int L, int64_t V);
int r4r_tower_span_fwd(const int32_t *tok, const int64_t *rev_off, const int64_t *first, const int64_t *nb,
                   int64_t owners, const int64_t *ids, int64_t n, int64_t group, int T, int R, int W, int64_t pad,
                   const float *table, int64_t V, const float *conv_w, const float *conv_b,
                   const float *fc_w, const float *fc_b, int E, int F, int L,
                   float *latent, int64_t *neigh, void *ws, size_t ws_bytes, int64_t *groups_done, void *stream);

/* ------------------------------------------------------------------------
 * Slates: the K best of, and the place of a target among, a per-query candidate LIST (csrc/slate_device.h).
 * A slate is the candidate list of one query: what a retrieval stage, a category filter or a basket hands to a
 * re-ranker, or the sampled negatives of a ranking metric.  The reference's only ranking metric is of the second kind,
 * HR@1 of one positive against five sampled negatives (eval.py:64-92, the rows built by data.py:375-447), one forward
 * per candidate; the calls below rank a positive against N given negatives at any K from the cached two sides, with
 * no forward at all, and order the K best of any list without a scan of the catalogue.
 *
 * <form> is one of dot, relu, hmlp, rfm, pfm; the leading arguments are exactly r4r_pair_<form>'s and score(u, i) is
 * that form's ONE fixed fp32 expression (the sections above), computed here as the scalar chain r4r_pair_<form> runs.
 *   Slates   slate s belongs to query row q_idx[s] (several slates may share a row); its entries are
 *            slate_ids[slate_off[s] .. slate_off[s + 1]), in any order.  The ids of one slate are distinct: the
 *            caller's duty, like the range of q_idx.  slate_off [n_s + 1] (r4r_slate_rank_<form>: [n_p + 1], one slate
 *            per pair).
 *   max_len  the caller's upper bound on a slate's length: the host knows it, and it spares a device read.  Understated,
 *            time is lost and no entry is: the last piece of a slate runs to the slate's end.
 *   Order    the existing one, in the existing words: score descending, ties by ascending id.  out_scores / out_score
 *            are r4r_pair_<form>'s bits.  An entry is never listed or counted when it is outside [0, n_c), on the
 *            ascending CSR exclusion list of the slate's query ROW (excl_off [n_q + 1], excl_ids; both NULL = none), or
 *            scored -inf or NaN.  Unused slots of a list hold id -1 and score -inf.
 *   Ranks    pair p = (query row q_idx[p], target t_idx[p], slate p): out_rank[p] = the number of entries != t of the
 *            slate that are ahead of t; the target need not be in the slate, and is never counted against itself.
 *            -1 for a target whose own score is -inf or NaN.  t_idx out of range is the caller's error.
 * The results depend on the inputs only: not on max_len, not on the order of the entries within a slate, not on which
 * slates share a call -- the order is total, a score's bits depend on its own pair only, ranks are integer atomics.
 * With slate = 0 .. n_c - 1 the lists and ranks are r4r_topk_<form>'s and r4r_rank_<form>'s, bit for bit.
 * Limits: 1 <= K <= 128, n_s, n_p, max_len >= 0, and the form's own width limits.  n_s == 0, n_p == 0 or n_c == 0
 * returns R4R_OK, enqueues nothing and leaves the outputs untouched.  Every refusal precedes the first launch and the
 * first dereference, in the entry point's own name; a short workspace is R4R_ERR_WORKSPACE; the grid product (slates x
 * pieces) is checked.  Nothing allocates, nothing synchronises.
 *
 * r4r_slate_piece: the entries one wave ranks at a time (a compile-time constant of the library; for callers and tests).
 * r4r_slate_ws_bytes: the partial lists [n_s, ceil(max_len / piece), K] of (score, id), 12 bytes each; 0 when max_len
 *   fits a single piece.
 * r4r_slate_topk_<form>: out_ids / out_scores [n_s, K].  One launch (a wave per slate and piece: the scores of the piece
 *   staged in LDS, a place = the count of entries ahead, places below K stored at their place), plus r4r_topk_dot's merge
 *   when a slate has several pieces.
 * r4r_slate_rank_<form>: out_rank / out_score [n_p].  Two launches: r4r_rank_<form>'s target kernel, then a wave per
 *   pair and piece that counts and adds one 64-bit integer atomic.  No workspace, no correction launch: exclusions are
 *   tested per entry.
 * Scored by scalar chains: for hmlp / rfm / pfm at their largest heads that is r4r_pair_<form>'s cost per entry (of the
 * order of 50 ms per 10^6 entries); scoring the entries 16 at a time in the columns of an MFMA tile is not built.
 * ---------------------------------------------------------------------- */
int r4r_slate_piece(void);
size_t r4r_slate_ws_bytes(int64_t n_s, int64_t max_len, int K);
int r4r_slate_topk_dot(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                       const float *c_bias, int D, const int64_t *q_idx, const int64_t *slate_off,
                       const int64_t *slate_ids, int64_t n_s, int64_t max_len, const int64_t *excl_off,
                       const int64_t *excl_ids, int K, void *ws, size_t ws_bytes, int64_t *out_ids, float *out_scores,
                       void *stream);
int r4r_slate_rank_dot(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                       const float *c_bias, int D, const int64_t *q_idx, const int64_t *t_idx, const int64_t *slate_off,
                       const int64_t *slate_ids, int64_t n_p, int64_t max_len, const int64_t *excl_off,
                       const int64_t *excl_ids, int64_t *out_rank, float *out_score, void *stream);
int r4r_slate_topk_relu(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                        const float *c_bias, const float *w, int H, int P, const int64_t *q_idx, const int64_t *slate_off,
                        const int64_t *slate_ids, int64_t n_s, int64_t max_len, const int64_t *excl_off,
                        const int64_t *excl_ids, int K, void *ws, size_t ws_bytes, int64_t *out_ids, float *out_scores,
                        void *stream);
int r4r_slate_rank_relu(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                        const float *c_bias, const float *w, int H, int P, const int64_t *q_idx, const int64_t *t_idx,
                        const int64_t *slate_off, const int64_t *slate_ids, int64_t n_p, int64_t max_len,
                        const int64_t *excl_off, const int64_t *excl_ids, int64_t *out_rank, float *out_score,
                        void *stream);
int r4r_slate_topk_hmlp(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                        const float *c_bias, const float *W, const float *b, const float *w, int D, int H,
                        const int64_t *q_idx, const int64_t *slate_off, const int64_t *slate_ids, int64_t n_s,
                        int64_t max_len, const int64_t *excl_off, const int64_t *excl_ids, int K, void *ws,
                        size_t ws_bytes, int64_t *out_ids, float *out_scores, void *stream);
int r4r_slate_rank_hmlp(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                        const float *c_bias, const float *W, const float *b, const float *w, int D, int H,
                        const int64_t *q_idx, const int64_t *t_idx, const int64_t *slate_off, const int64_t *slate_ids,
                        int64_t n_p, int64_t max_len, const int64_t *excl_off, const int64_t *excl_ids,
                        int64_t *out_rank, float *out_score, void *stream);
int r4r_slate_topk_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                       const float *c_bias, const float *W, const float *b, const float *s, const float *l, int H, int P,
                       int M, const int64_t *q_idx, const int64_t *slate_off, const int64_t *slate_ids, int64_t n_s,
                       int64_t max_len, const int64_t *excl_off, const int64_t *excl_ids, int K, void *ws,
                       size_t ws_bytes, int64_t *out_ids, float *out_scores, void *stream);
int r4r_slate_rank_rfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                       const float *c_bias, const float *W, const float *b, const float *s, const float *l, int H, int P,
                       int M, const int64_t *q_idx, const int64_t *t_idx, const int64_t *slate_off,
                       const int64_t *slate_ids, int64_t n_p, int64_t max_len, const int64_t *excl_off,
                       const int64_t *excl_ids, int64_t *out_rank, float *out_score, void *stream);
int r4r_slate_topk_pfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                       const float *c_bias, const float *W, const float *b, const float *s, const float *g, const float *e,
                       int H, int G, int M, const int64_t *q_idx, const int64_t *slate_off, const int64_t *slate_ids,
                       int64_t n_s, int64_t max_len, const int64_t *excl_off, const int64_t *excl_ids, int K, void *ws,
                       size_t ws_bytes, int64_t *out_ids, float *out_scores, void *stream);
int r4r_slate_rank_pfm(const float *q, int64_t n_q, const float *q_bias, const float *c, int64_t n_c, int64_t c_stride,
                       const float *c_bias, const float *W, const float *b, const float *s, const float *g, const float *e,
                       int H, int G, int M, const int64_t *q_idx, const int64_t *t_idx, const int64_t *slate_off,
                       const int64_t *slate_ids, int64_t n_p, int64_t max_len, const int64_t *excl_off,
                       const int64_t *excl_ids, int64_t *out_rank, float *out_score, void *stream);

/* ------------------------------------------------------------------------
 * NARRE explanations: the eval-mode review attention that KEEPS its weights (csrc/narre_explain.hip).
 * NARRE is rating regression "with review-level explanations": the attention of NARRE.attention, NARRE.py:53-64, says
 * which reviews of an item (which of a user's own reviews) carry a prediction.  r4r_narre_attn_fwd saves the weights as
 * backward state only and stops at 32 x 32; this call is forward only, reaches every R and L in 1..64, gathers the
 * neighbour rows by id (no [N, R, L] `other` block is built), adds the owner's own row and lists the K heaviest REAL
 * reviews of every owner.  The arithmetic is r4r_narre_attn_fwd's with mult = NULL:
 *   h      = relu(W0 [z_r ; other_table[nb_r]] + b0)      W0 [L, 2L]; b0 [L]; w3 [L]; b3 [1]
 *   a      = softmax_R(w3 . h + b3)                        padded reviews are NOT masked out of the softmax
 *   out[n] = sum_r a[n, r] z[n, r, :]  (+ own_table[owner[n]])
 * An nb id outside [0, other_rows) reads as a row of zeros: no id makes the kernel read outside other_table.  owner[n]
 * is a row of own_table, whose height the call is not told: its range is the caller's duty, like q_idx elsewhere.
 *   Lists   slot r of owner n is listed only if r < live[n] (live NULL: every slot; a value outside 0..R is clamped):
 *           weight descending, ties by ascending slot; top_w holds the bits of attn[n, slot] -- the model's own weights,
 *           not renormalised over the live slots.  A place is the count of live slots ahead (R <= 64 is one wave's worth
 *           of slots).  Places beyond min(K, live[n]) hold (-1, 0.0f).
 * An owner's out, attn and list depend on that owner's inputs and the weights only: not on N, not on which owners share
 * a call, not on K, not on which outputs are NULL.  A slot's logit depends on that slot's inputs only, by one instruction
 * sequence for every slot: slots with equal z rows and equal neighbour ids get equal bits.
 * Limits: 1 <= R <= 64, 1 <= L <= 64, 0 <= K <= R, N >= 0, other_rows >= 0.  own_table and owner both or neither,
 * top_slot and top_w both or neither (K > 0 needs them), at least one output.  N == 0 returns R4R_OK and enqueues
 * nothing.  Every refusal precedes the launch and the first dereference, in the entry point's own name.  One launch;
 * nothing allocates, nothing synchronises.
 * ---------------------------------------------------------------------- */
int r4r_narre_explain(const float *z,            /* [N, R, L] review latents                              */
                      const int64_t *nb,         /* [N, R] neighbour ids, rows of other_table             */
                      const float *other_table, int64_t other_rows,   /* [other_rows, L]                  */
                      const float *own_table, const int64_t *owner,   /* [*, L], [N]; both NULL: no add   */
                      const int32_t *live,       /* [N] real reviews of the owner, 0..R; NULL: all R      */
                      const float *W0, const float *b0, const float *w3, const float *b3,
                      float *out,                /* [N, L]  sum_r a_r z_r (+ own_table[owner]); may be NULL */
                      float *attn,               /* [N, R]  softmax weights, padded slots included; may be NULL */
                      int32_t *top_slot, float *top_w, int K,         /* [N, K] each; K = 0: both NULL    */
                      int64_t N, int R, int L, void *stream);

/* ------------------------------------------------------------------------
 * Phrase explanations: the word windows that win a TextCNN tower's max-pool (csrc/phrases.hip, csrc/tower_span.hip).
 * Every tower is conv 3 x E (pad 2) -> ReLU -> global max-pool (common_pytorch_models.py:29-31): filter f of a document
 * contributes the activation of ONE three-word window, the one at argmax[n, f], and an owner's latent vector is a
 * linear image of those F numbers -- DeepCoNN.py:53-54, NARRE.py:95-96 (per review), TransNet.py:100-102.  Nothing else
 * of the document reaches the prediction, so "which phrases carry this vector" has a model-faithful answer, and
 * r4r_textcnn_fwd already returns it: pooled [N, F] and argmax [N, F].  These calls list it; nothing is recomputed.
 *   Live     filter f of row n is live iff 0 <= argmax[n, f] < T + 2 (the conv's output positions).  Anything else is
 *            dead and contributes nothing: -1 (what the conv writes where pooled == 0) included.
 *   Window   the window of a live filter is its position p = argmax[n, f]; it covers the words p - 2 .. p of the row.
 *   Score    over the live filters with that position in ASCENDING f, starting from 0.0f:
 *            wt == NULL: acc = acc + pooled[n, f] (plain fp32 adds); else acc = fmaf(wt[n * wt_stride + f], pooled[n, f],
 *            acc).  wt_stride 0: one [F] vector for every row; wt_stride F: [N, F].  Finite weights are the caller's duty.
 *   Lists    a row's distinct windows, score descending, ties by ascending position: top_pos, top_score (the bits of
 *            the chain above), top_filters (the number of live filters the window won).  A place is the count of windows
 *            ahead; F <= 112 is two filters per lane of one wave.  Entries min(K, windows) .. K hold (-1, 0.0f, 0).
 *            n_windows[n] = the number of distinct windows, 0 for a row of dead filters.
 *   Tokens   top_tok[n, k, j] = idx[n, p - 2 + j] where 0 <= p - 2 + j < T, else -1: -1 is the conv's zero padding, as
 *            distinct from the pad word id 0.  A fill entry is three -1.
 * A row's outputs depend on that row's inputs only: not on N, not on which rows share a call, not on which outputs are
 * NULL; the list at K is the first K entries of the list at any larger K.
 *
 * r4r_textcnn_phrases: ONE launch.  Refused before it, in the entry point's name: null pooled / argmax, F outside
 *   1 .. 112, K outside 1 .. F, T < 1, N < 0 or N >= 2^31, wt_stride other than 0 or F, top_tok without idx.  N == 0
 *   returns R4R_OK and enqueues nothing.  Every output is nullable.
 * r4r_tower_span_phrases: r4r_tower_span_fwd's rounds (the same pools, ids, group, T / R / W / pad, table, conv
 *   arguments and workspace: r4r_tower_span_ws_bytes, which alone is told a latent size) with the lists in the place of
 *   the latents.  Round g enqueues r4r_tower_build, r4r_textcnn_fwd over the round's rows and r4r_textcnn_phrases over
 *   the round's pooled / argmax / documents (T = the row's width: input_length, or W with R > 0) into the round's slice
 *   of the outputs, which hold one row per document: n rows, or n R rows in the span's order with R > 0.  With
 *   wt_stride == F the weights are indexed by the span's global row.  neigh [n, 10] is r4r_tower_build's, needed with
 *   R > 0.  A span over `group` gives the bits of one host-built chunk + r4r_textcnn_fwd + r4r_textcnn_phrases call per
 *   chunk of `group` owners.  Refusals, groups_done, n == 0: r4r_tower_span_fwd's, plus K and wt_stride as above and
 *   n max(R, 1) >= 2^31.  Nothing allocates, nothing synchronises, no training state is touched.
 * ---------------------------------------------------------------------- */
int r4r_textcnn_phrases(const float *pooled, const int32_t *argmax,   /* [N, F] as r4r_textcnn_fwd wrote them        */
                        const float *wt, int64_t wt_stride,           /* NULL = 1; stride 0: [F]; stride F: [N, F]    */
                        const int64_t *idx,                           /* [N, T] the documents; only for top_tok       */
                        int64_t N, int T, int F, int K,
                        int32_t *top_pos, float *top_score, int32_t *top_filters,   /* [N, K] each, nullable          */
                        int64_t *top_tok,                             /* [N, K, 3], nullable; needs idx               */
                        int32_t *n_windows,                           /* [N], nullable                                */
                        void *stream);
int r4r_tower_span_phrases(const int32_t *tok, const int64_t *rev_off, const int64_t *first, const int64_t *nb,
                           int64_t owners, const int64_t *ids, int64_t n, int64_t group, int T, int R, int W, int64_t pad,
                           const float *table, int64_t V, const float *conv_w, const float *conv_b, int E, int F,
                           const float *wt, int64_t wt_stride, int K,
                           int32_t *top_pos, float *top_score, int32_t *top_filters, int64_t *top_tok, int32_t *n_windows,
                           int64_t *neigh, void *ws, size_t ws_bytes, int64_t *groups_done, void *stream);

/* ------------------------------------------------------------------------
 * Pair gradients: the model's prediction for explicit (user, item) pairs, its gradient with respect to the two tower
 * latents, and that gradient carried back to each tower's pooled features (csrc/pair_grad.hip).  The last is the
 * per-row filter weight r4r_textcnn_phrases takes (wt_stride == F): the windows listed with it are the words behind ONE
 * pair's score, not behind an owner.  One launch over the model's RAW head parameters; nothing is folded.
 *   zu [n_u, L], zi [n_i, L]  the eval-mode tower outputs z = fc.weight pooled + fc.bias (the dropout of
 *                             common_pytorch_models.py:37 is the identity in eval mode); x = [zu[u_idx[p]] ; zi[i_idx[p]]]
 *   fc_u, fc_i [L, F]         the towers' fc.weight:  w_user[p, f] = sum_l g_user[p, l] fc_u[l, f], w_item likewise
 *   q_bias [n_u], c_bias [n_i]  every scalar of the score (bias tables, global bias, lin.bias, final.3.bias), indexed as
 *                             zu / zi are; NULL counts as 0: the convention of r4r_pair_<form>
 *   kind R4R_PAIR_GRAD_FM -- deepconn (DeepCoNN.py:61-66; TorchFM, common_pytorch_models.py:49-57).  V [2L, 8], lw [2L]:
 *     s_k = sum_j x_j V_jk      score = q_bias + c_bias + sum_j lw_j x_j + 1/2 (sum_k s_k^2 - sum_j x_j^2 sum_k V_jk^2)
 *     g_j = lw_j + sum_k s_k V_jk - x_j sum_k V_jk^2
 *   kind R4R_PAIR_GRAD_MLP -- deepconn++ (DeepCoNN.py:68-72).  W0 [L, 2L], b0 [L], w3 [L]:
 *     a = W0 x + b0             score = sum_m w3_m max(a_m, 0) + q_bias + c_bias
 *     g_j = sum_m [a_m > 0] w3_m W0[m, j]                       (the ReLU's derivative at 0 is 0, as in torch)
 *   kind R4R_PAIR_GRAD_PFM -- transnet / transnet++ at test time (TransNet.py:25-35, 105-114).  W0, b0 as above,
 *     W2 [L, L], b2 [L], V [2P + L, 8], lw [2P + L]; xu [*, P], xi [*, P] the id-embedding tables, rows u_idx / i_idx
 *     (P = 5 for transnet++, TransNet.py:75-76, 108-110; P = 0: no row is read and xu, xi may be NULL):
 *     a = W0 x + b0, ir = W2 max(a, 0) + b2, y = [xu[u] ; xi[i] ; ir]; the score is the fm expression over y, gy the fm
 *     gradient over y, and g = W0^T ([a > 0] o (W2^T gy[2P:])).
 * Fixed fp32 order (one wave per pair; "chain": fmaf accumulation from 0.0f in ascending index):
 *   rows   a_m (and ir_m): 16 lanes per m, lane c chains j = c, c + 16, ..; the 16 partials are added by the steps
 *          xor 1, xor 2, rotate 4, rotate 8 within the 16 (v += partner each time); then + b_m.
 *   cols   g_j = chain over m of upstream_m W0[m, j]; W2^T gy and w = g fc likewise (chain over the row index).  A
 *          masked unit enters the chain as 0.0f.
 *   fm     lane (jg, k), jg = lane / 8, k = lane % 8, chains j = jg, jg + 8, ..; s_k = ((p_0k + p_1k) + ..) + p_7k.
 *          Per j: v2_j = chain over k of V_jk^2, dot_j = chain over k of s_k V_jk, g_j = fmaf(-x_j, v2_j, lw_j + dot_j).
 *          lin = wave sum of the lanes' chains (j = lane, lane + 64, ..) of lw_j x_j; q2 likewise of fmaf(x_j x_j, v2_j, .)
 *          with x_j x_j rounded first; wave sum = the four steps above, then (r_0 + r_16) + (r_32 + r_48) over the four
 *          16-lane totals.  ss = chain over k of s_k^2.  fm = fmaf(0.5f, ss - q2, lin).
 *   mlp    score's sum = wave sum of w3_m max(a_m, 0), lane = m.
 *   score  out_score = (head + q_bias) + c_bias.
 * A pair's outputs depend on that pair's inputs only: not on n_p, not on which pairs share the call, not on the grid, not
 * on which outputs are NULL; the same pair gives the same bits alone, inside a batch and in a permuted batch.
 * Limits: fm 1 <= L <= 128; mlp, pfm 1 <= L <= 64 (the native steps' limits); 0 <= P <= 8 (0 unless pfm);
 * 1 <= F <= 112; n_u, n_i >= 0; 0 <= n_p < 2^31.  Refused before the launch and before the first dereference, in the
 * entry point's own name: an unknown kind, a limit above, a null pointer among the kind's parameters (xu / xi with
 * P > 0), w_user without fc_u, w_item without fc_i and, with n_p > 0, null zu / zi / u_idx / i_idx or n_u / n_i == 0.
 * n_p == 0 returns R4R_OK and enqueues nothing.  Every output may be NULL.  An index outside [0, n_u) / [0, n_i) is the
 * caller's error, as in r4r_pair_dot.  Nothing allocates, nothing synchronises.
 * ---------------------------------------------------------------------- */
#define R4R_PAIR_GRAD_FM 0
#define R4R_PAIR_GRAD_MLP 1
#define R4R_PAIR_GRAD_PFM 2
int r4r_pair_grad(int kind, const float *zu, int64_t n_u, const float *zi, int64_t n_i,
                  const int64_t *u_idx, const int64_t *i_idx, int64_t n_p,     /* [n_p] rows of zu / zi             */
                  const float *q_bias, const float *c_bias,                     /* [n_u], [n_i]; NULL = 0            */
                  const float *W0, const float *b0, const float *W2, const float *b2, const float *w3,
                  const float *V, const float *lw,
                  const float *xu, const float *xi, int P,                      /* pfm's id embeddings [*, P]        */
                  const float *fc_u, const float *fc_i, int L, int F,           /* [L, F] each                       */
                  float *out_score,                                             /* [n_p], nullable                   */
                  float *g_user, float *g_item,                                 /* [n_p, L] each, nullable           */
                  float *w_user, float *w_item,                                 /* [n_p, F] each, nullable           */
                  void *stream);

/* ------------------------------------------------------------------------
 * NARRE pair gradients: the reviews and the words behind ONE user-item score of NARRE (csrc/narre_pair.hip).  NARRE's
 * review latents reach the score through the softmax of the review attention (NARRE.attention, NARRE.py:53-64; the
 * scorer of NARRE.py:24-36), so the gradient of a score with respect to a review's pooled features has a direct part
 * (through a_r z_r) and a part through the review's logit.  It splits into a pass per OWNER, which does all the matrix
 * work of a review once, and a pass per PAIR, which is two L x L and two L x F matvecs plus O(R (L + F)) combining.
 * One side (user or item), eval mode, with z_r = fc pooled_r + fc.bias, fc [L, F] the side's tower fc.weight:
 *   pre_r = W0 [z_r ; other_table[nb_r]] + b0     a = softmax_R(w3 . relu(pre_r) + b3)     o = sum_r a_r z_r
 *   p = o + own_table[owner]
 * The head (NARRE.py:38-46, 115-124; dropout is the identity in eval mode): x = p_u o p_i, t = W1 x + b1 (final.1),
 * score = w . relu(t) + scalars (final.3 and the three biases).
 *   per pair    gx = W1^T ([t > 0] o w),  g_u = gx o p_i,  g_i = gx o p_u;  per side with its g:
 *               ga_r = g . z_r,  dot = sum_r a_r ga_r,  delta_r = a_r (ga_r - dot)  (= d score / d logit_r; sums to 0)
 *   per owner   D_r = sum_m [pre_rm > 0] w3_m W0[m, 0:L]   [R, L]   (the ReLU's derivative at 0 is 0, as in torch)
 *               E_r = D_r fc   [R, F]          dz_r = D_r . z_r   [R]
 *   result      w[r, f] = d score / d pooled[r, f] = a_r (g fc)_f + delta_r E[r, f]: the per-review filter weights
 *               r4r_textcnn_phrases takes (wt_stride == F, one row per review)
 *               rev_r = a_r ga_r + delta_r dz_r  (gradient . input): how much review r carries THIS pair's score
 *
 * r4r_narre_attn_jac -- the owner pass: r4r_narre_explain's inputs plus fc; one wave per owner, one launch.
 *   attn, out   r4r_narre_explain's bits for the same inputs (the same instruction sequence); pooled_attn is out before
 *               the own row is added (o above).  An nb id outside [0, other_rows) reads as a row of zeros.
 *   Fixed fp32 order of the new outputs ("chain": fmaf accumulation from 0.0f in ascending index):
 *     D[r, j]   chain over m of c_m W0[m, j], c_m = w3_m where pre_rm > 0 (the bits of r4r_narre_explain's pre), else
 *               0.0f: a masked unit enters the chain as 0.0f
 *     dz[r]     wave sum over the lanes j of D[r, j] z[r, j] (the product rounded; 0 in the lanes past L): the steps
 *               xor 1, xor 2, rotate 4, rotate 8 within each 16 lanes, then (r_0 + r_16) + (r_32 + r_48)
 *     E[r, f]   chain over l of D[r, l] fc[l, f]
 *   An owner's outputs depend on that owner's inputs and the weights only: not on N, not on which owners share a call,
 *   not on which outputs are NULL.  Limits: 1 <= R <= 64, 1 <= L <= 64, 1 <= F <= 112, N >= 0, other_rows >= 0;
 *   own_table and owner both or neither; E needs fc; at least one output.  N == 0 returns R4R_OK and enqueues nothing.
 *
 * r4r_narre_pair_grad -- the pair pass over the owner pass's outputs of both sides (p = its `out`); one wave per pair,
 *   one launch.  The two sides may have different R.  Fixed fp32 order:
 *     x_l = p_u[l] p_i[l];  t_m: "rows" of the Pair gradients section (16 lanes per m, lane c chains j = c, c + 16, ..,
 *     the steps xor 1, xor 2, rotate 4, rotate 8, then + b1_m);  head = wave sum of w_m max(t_m, 0), lane = m;
 *     gx_j = chain over m of ([t_m > 0] w_m) W1[m, j];  g_u[l] = gx_l p_i[l],  g_i[l] = gx_l p_u[l]
 *     ga_r: "rows" over z_r without a bias;  dot = chain over r of a_r ga_r;  delta_r = a_r (ga_r - dot): exactly 0 at
 *     R == 1 (a_0 == 1.0f);  b_f = chain over l of g_l fc[l, f]
 *     w[r, f] = fmaf(delta_r, E[r, f], a_r b_f)        rev_r = fmaf(delta_r, dz_r, a_r ga_r)   (products rounded first)
 *     out_score = (head + q_bias) + c_bias;  q_bias [n_u] / c_bias [n_i] hold every scalar of the score, NULL counts as 0
 *   A pair's outputs depend on that pair's inputs only: not on n_p, the grid, the other pairs or which outputs are NULL;
 *   the same pair gives the same bits alone, inside a batch and in a permuted batch.  Every output is indexed with 64-bit
 *   offsets; a pair's [R, F] block is stored contiguously by full waves.
 *   Limits: the owner pass's for R_u, R_i, L, F; n_u, n_i >= 0; 0 <= n_p < 2^31.  Refused before the launch and the first
 *   dereference, in the entry point's own name: a limit; w_user without fc_u or E_u, rev_user without dz_u, any of
 *   glogit_user / rev_user / w_user without z_u and attn_u (the item side likewise); with n_p > 0 a null p_u, p_i,
 *   u_idx, i_idx, W1, b1 or w, and n_u or n_i == 0.  n_p == 0 returns R4R_OK and enqueues nothing.  An index outside
 *   [0, n_u) / [0, n_i) is the caller's error.  Nothing allocates, nothing synchronises.
 * ---------------------------------------------------------------------- */
int r4r_narre_attn_jac(const float *z,            /* [N, R, L] review latents                              */
                       const int64_t *nb,         /* [N, R] neighbour ids, rows of other_table             */
                       const float *other_table, int64_t other_rows,   /* [other_rows, L]                  */
                       const float *own_table, const int64_t *owner,   /* [*, L], [N]; both NULL: no add   */
                       const float *W0, const float *b0, const float *w3, const float *b3,
                       const float *fc, int F,    /* [L, F] the side's tower fc.weight; needed for E       */
                       float *attn,               /* [N, R]  softmax weights; nullable                     */
                       float *pooled_attn,        /* [N, L]  o, without the own row; nullable              */
                       float *out,                /* [N, L]  p = o + own_table[owner]; nullable            */
                       float *D,                  /* [N, R, L] nullable                                    */
                       float *E,                  /* [N, R, F] nullable                                    */
                       float *dz,                 /* [N, R]  nullable                                      */
                       int64_t N, int R, int L, void *stream);
int r4r_narre_pair_grad(const float *p_u, const float *z_u, const float *attn_u, const float *E_u, const float *dz_u,
                        const float *fc_u, int64_t n_u, int R_u,     /* [n_u, L], [n_u, R_u, L], [n_u, R_u], [n_u, R_u, F], [n_u, R_u], [L, F] */
                        const float *p_i, const float *z_i, const float *attn_i, const float *E_i, const float *dz_i,
                        const float *fc_i, int64_t n_i, int R_i,     /* the item side likewise                */
                        const int64_t *u_idx, const int64_t *i_idx, int64_t n_p,    /* [n_p] rows of the sides   */
                        const float *q_bias, const float *c_bias,                    /* [n_u], [n_i]; NULL = 0    */
                        const float *W1, const float *b1, const float *w, int L, int F,   /* [L, L], [L], [L]     */
                        float *out_score,                                            /* [n_p], nullable           */
                        float *g_user, float *g_item,                                /* [n_p, L] each, nullable   */
                        float *glogit_user, float *glogit_item,                      /* [n_p, R_u] / [n_p, R_i]   */
                        float *rev_user, float *rev_item,                            /* [n_p, R_u] / [n_p, R_i]   */
                        float *w_user, float *w_item,                   /* [n_p, R_u, F] / [n_p, R_i, F], nullable */
                        void *stream);

/* ------------------------------------------------------------------------
 * NARRE what-if scores: a pair's eval-mode rating with chosen reviews of either owner REMOVED (csrc/narre_whatif.hip).
 * A review enters NARRE's score only through its own latent z_r and its own attention logit (NARRE.attention,
 * NARRE.py:53-64; the scorer of NARRE.py:24-36), so "what would the model predict without review r" needs no tower:
 * the loader's own removal (`skip`, data.py:144-172 for the reviews, data.py:275-279 for the neighbour ids: slot r holds
 * the r-th REMAINING review, the next review beyond R slides in, padding fills the tail) is a re-selection of slots, a new
 * softmax and a new pooled vector.  An owner pass returns every slot's logit once; a variant pass scores
 * n_p pairs x V variants.
 *
 * r4r_narre_logits -- the owner pass over S slots per owner: r4r_narre_explain's attention inputs, one wave per owner, one
 *   launch.  logit[n, s] = w3 . relu(W0 [z[n, s] ; other_table[nb[n, s]]] + b0) + b3, the PRE-softmax value, by
 *   r4r_narre_explain's instruction sequence: lane l chains column c ascending of W0[l, c] cat[c] from 0.0f, + b0[l],
 *   relu; the sum over l of w3_l h_l (the product rounded) is the wave sum of the Pair gradients section (xor 1, xor 2,
 *   rotate 4, rotate 8 within each 16 lanes, then (r_0 + r_16) + (r_32 + r_48)), then + b3.  A slot's logit depends on
 *   that slot's inputs only: equal z rows and equal ids give equal bits, whatever N, S, the slot index and who shares the
 *   call.  An nb id outside [0, other_rows) reads as a row of zeros.  Limits: 1 <= S <= 64, 1 <= L <= 64, N >= 0,
 *   other_rows >= 0.  N == 0 returns R4R_OK and enqueues nothing.  The padding slot of a side is the call with N = 1,
 *   S = 1 on z_pad (the tower on an all-padding review) and the pad id (total + 1 of the other side, data.py:275-276).
 *
 * r4r_narre_whatif -- the variant pass; one wave per (pair, 16 variants), one launch.  Per side: z [n, S, L] and
 *   logit [n, S] (the owner pass's), own [n, L] (the owners' id-embedding rows, NARRE.py:115-116; NULL = no add),
 *   z_pad [L], logit_pad, and R, the slots the model attends, 1 <= R <= S <= 64; the sides may differ in R and S.
 *   drop_u, drop_i [n_p, V] int64 bit masks, bit s = slot s removed (NULL = nothing removed).
 *   One (pair, variant, side):
 *     list   the first R slots of 0 .. S - 1 whose bit is clear, in ascending slot order; with fewer than R left the tail
 *            is copies of the pad slot (logit_pad, z_pad).  Bits at positions >= S are ignored.  With S = R + (drops)
 *            this is the loader's `skip` rule; with S = R it is occlusion by padding.
 *     a'     lane k holds the k-th selected logit: m = wave max, e_k = expf(logit_k - m), den = wave sum of e (the order
 *            above, 0.0f in the lanes past R), a'_k = e_k / den
 *     o'_l   chain over k ascending of fmaf(a'_k, z'_k[l], .) from 0.0f;   p'_l = o'_l + own[l] (no add with a NULL own)
 *   The head (NARRE.py:38-46, 115-124; dropout is the identity in eval mode): x_l = p'_u[l] p'_i[l];
 *     t_j = chain over l ascending of fmaf(W1[j, l], x_l, .) from 0.0f (v_mfma_f32_16x16x4_f32, bitwise that chain; the
 *     variants are its columns);  z_j = fmaxf(t_j + b1_j, 0);  h_g = chain of fmaf(w_j, z_j, .) over the j with
 *     ((j >> 2) & 3) == g, ascending;  head = (h_0 + h_1) + (h_2 + h_3);  out_score[p, v] = (head + q_bias[u]) + c_bias[i]
 *     (q_bias [n_u] / c_bias [n_i] hold every scalar of the score; NULL counts as 0).
 *   A variant's bits depend only on its own pair's inputs, the ordered selected list and the pad count: not on V, the
 *   variant's column, n_p, the grid, the other variants or how the mask spells the same list (a bit on a slot that would
 *   not have been selected changes nothing).
 *   Limits: 1 <= L <= 64, V >= 1, n_u, n_i >= 0, 0 <= n_p, n_p V < 2^31.  Refused before the launch and the first
 *   dereference, in the entry point's own name: a limit; with n_p > 0 a null z, logit, z_pad of either side, u_idx,
 *   i_idx, W1, b1, w or out_score, and n_u or n_i == 0.  n_p == 0 returns R4R_OK and enqueues nothing.  An index outside
 *   [0, n_u) / [0, n_i) is the caller's error.  Both calls: one launch; nothing allocates, nothing synchronises.
 * ---------------------------------------------------------------------- */
int r4r_narre_logits(const float *z,              /* [N, S, L] review latents                              */
                     const int64_t *nb,           /* [N, S] neighbour ids, rows of other_table             */
                     const float *other_table, int64_t other_rows,   /* [other_rows, L]                    */
                     const float *W0, const float *b0, const float *w3, const float *b3,
                     float *logit,                /* [N, S]  the pre-softmax logits                        */
                     int64_t N, int S, int L, void *stream);
int r4r_narre_whatif(const float *z_u, const float *logit_u, const float *own_u, const float *z_pad_u, float logit_pad_u,
                     int64_t n_u, int S_u, int R_u,          /* [n_u, S_u, L], [n_u, S_u], [n_u, L] or NULL, [L]      */
                     const float *z_i, const float *logit_i, const float *own_i, const float *z_pad_i, float logit_pad_i,
                     int64_t n_i, int S_i, int R_i,          /* the item side likewise                                */
                     const int64_t *u_idx, const int64_t *i_idx,              /* [n_p] rows of the sides              */
                     const int64_t *drop_u, const int64_t *drop_i,            /* [n_p, V] bit masks; NULL = 0         */
                     int64_t n_p, int V,
                     const float *q_bias, const float *c_bias,                /* [n_u], [n_i]; NULL = 0               */
                     const float *W1, const float *b1, const float *w, int L, /* [L, L], [L], [L]                     */
                     float *out_score,                                        /* [n_p, V]                             */
                     void *stream);

/* ------------------------------------------------------------------------
 * NARRE counterfactual search: the fewest reviews whose removal moves a pair's eval-mode rating past a target, by a
 * greedy search that runs whole on the device (csrc/narre_search.hip).  A review enters NARRE's score only through its
 * own latent and its own attention logit (NARRE.attention, NARRE.py:53-64; the head of NARRE.py:38-46, 115-124), and a
 * removal is the loader's own (`skip`, data.py:144-172 for the reviews, data.py:275-279 for the neighbour ids), so every
 * candidate removal at every step is one variant of "NARRE what-if scores": no tower runs, the owner pass
 * (r4r_narre_logits) is paid once.
 *
 * r4r_narre_search -- one launch, one wave per pair for the pair's whole search.  Per side exactly r4r_narre_whatif's
 *   block: z [n, S, L], logit [n, S], own [n, L] or NULL, z_pad [L], logit_pad, S, R with 1 <= R <= S <= 64; u_idx, i_idx
 *   [n_p]; q_bias, c_bias (NULL = 0); W1, b1, w; 1 <= L <= 64.
 *   start_u, start_i [n_p] int64 (NULL = 0): the slots already removed before the search; bits >= S are ignored.
 *   cand_u, cand_i   [n_p] int64 (NULL = no candidate on that side): the slots the search may remove; bits >= S and
 *                    bits that are also in start are ignored.
 *   target [n_p] float and direction: 0 = push down, done when score < target; 1 = push up, done when score > target.
 *                    Strict float compares: a NaN target never ends a search early, an equal score does not cross.
 *   budget B, 1 <= B <= 64: the most removals of one pair.
 *   The rule, per pair.  The masks start at start; out_scores[p, 0] is the score under them.  If it satisfies the
 *   comparison the pair is done with 0 removals.  Otherwise, at each step, the candidates are the slots that are set in
 *   cand, not yet removed and CURRENTLY SELECTED: among the first R clear slots of their side (a review the model does
 *   not attend cannot change the score, so it is never a step).  Candidate numbers: c = slot on the user side,
 *   c = 64 + slot on the item side.  Each candidate's score is the score with that one more bit set; the step takes the
 *   lowest score (direction 0) or the highest (direction 1), ties (float ==) to the lowest c, a NaN score never over a
 *   number (all NaN: the lowest c).  The best candidate is taken even when it moves the score the wrong way: a search,
 *   not a descent with early stopping.  The search ends when the comparison holds, after B removals, or when no
 *   candidate is left.
 *   out_order   [n_p, B] int32      c per step; -1 beyond the last step
 *   out_scores  [n_p, B + 1] float  the score after each step; the columns beyond the last step repeat the last score
 *   out_steps   [n_p] int32         the removals made
 *   out_crossed [n_p] int32         1 when the last score satisfies the comparison, else 0
 *   Bits: a score is r4r_narre_whatif's out_score of the same pair under the same two masks, bit for bit -- the list,
 *   a', o', p', x, the v_mfma_f32_16x16x4_f32 chain, the epilogue and (head + q_bias[u]) + c_bias[i] of that section
 *   (the pooling is one function both kernels call, csrc/narre_variant_device.h).  A pair's outputs depend on its own
 *   inputs only: not on n_p, the grid or which pairs share the call, and on budget by truncation only -- a search at
 *   budget B is the prefix of the same search at B' > B.
 *   Limits: 1 <= L <= 64, 1 <= B <= 64, direction 0 or 1, n_u, n_i >= 0, 0 <= n_p, n_p (B + 1) < 2^31.  Refused before
 *   the launch and the first dereference, in the entry point's own name: a limit; with n_p > 0 a null z, logit, z_pad of
 *   either side, u_idx, i_idx, target, W1, b1, w or output, and n_u or n_i == 0.  n_p == 0 returns R4R_OK and enqueues
 *   nothing.  An index outside [0, n_u) / [0, n_i) is the caller's error.  One launch; nothing allocates, nothing
 *   synchronises.
 * ---------------------------------------------------------------------- */
int r4r_narre_search(const float *z_u, const float *logit_u, const float *own_u, const float *z_pad_u, float logit_pad_u,
                     int64_t n_u, int S_u, int R_u,          /* [n_u, S_u, L], [n_u, S_u], [n_u, L] or NULL, [L]      */
                     const float *z_i, const float *logit_i, const float *own_i, const float *z_pad_i, float logit_pad_i,
                     int64_t n_i, int S_i, int R_i,          /* the item side likewise                                */
                     const int64_t *u_idx, const int64_t *i_idx,              /* [n_p] rows of the sides              */
                     const int64_t *start_u, const int64_t *start_i,          /* [n_p] bit masks; NULL = 0            */
                     const int64_t *cand_u, const int64_t *cand_i,            /* [n_p] bit masks; NULL = 0            */
                     const float *target, int direction, int budget,          /* [n_p]; 0 down / 1 up; 1 .. 64        */
                     int64_t n_p,
                     const float *q_bias, const float *c_bias,                /* [n_u], [n_i]; NULL = 0               */
                     const float *W1, const float *b1, const float *w, int L, /* [L, L], [L], [L]                     */
                     int32_t *out_order, float *out_scores,                   /* [n_p, B], [n_p, B + 1]               */
                     int32_t *out_steps, int32_t *out_crossed,                /* [n_p] each                           */
                     void *stream);

/* ------------------------------------------------------------------------
 * NARRE Shapley values: how much of a pair's eval-mode rating each review carries, as the exact Shapley value of the game
 * "which of the players' reviews are present" (csrc/narre_shapley.hip).  A review enters NARRE's score only through its
 * own latent and its own attention logit (NARRE.attention, NARRE.py:53-64; the head of NARRE.py:38-46, 115-124), and an
 * absent review is the loader's own removal (`skip`, data.py:144-172 for the reviews, data.py:275-279 for the neighbour
 * ids), so a coalition is one variant of "NARRE what-if scores": no tower runs, the owner pass (r4r_narre_logits) is
 * paid once.  No mask and no score of a coalition goes through memory unless out_values asks for the scores.
 *
 * r4r_narre_shapley -- one wave per (pair, 1,024 coalitions).  Per side exactly r4r_narre_whatif's block: z [n, S, L],
 *   logit [n, S], own [n, L] or NULL, z_pad [L], logit_pad, S, R with 1 <= R <= S <= 64; u_idx, i_idx [n_p]; q_bias, c_bias
 *   (NULL = 0); W1, b1, w; 1 <= L <= 64.
 *   start_u, start_i [n_p] int64 (NULL = 0): the slots removed in EVERY coalition; bits >= S are ignored (as in
 *                    r4r_narre_search).
 *   play_u, play_i   [n_p] int64 (NULL = no player on that side): the players; bits >= S and bits that are also in start
 *                    are ignored.  Player numbers t = 0 .. n - 1 run over the user side's player slots ascending, then
 *                    the item side's.
 *   P, 1 <= P <= 16: the most players of a pair; a pair with more set bits plays its lowest-numbered P.  out_n returns
 *                    the count played.
 *   Coalition c in [0, 2^n) has bit t set when player t is PRESENT; its masks are start | (the players whose bit in c is
 *   clear) on each side, and its value v(c) is r4r_narre_whatif's out_score of the pair under those two masks, bit for
 *   bit -- the list, a', o', p', x, the v_mfma_f32_16x16x4_f32 chain, the epilogue and (head + q_bias[u]) + c_bias[i] of
 *   that section, through the same calls (csrc/narre_variant_device.h's variant_pooled and variant_head).  v(2^n - 1) is
 *   the pair's score under start alone.
 *   phi_t = sum over c of coef_t(c) (v(c) - v(2^n - 1)), coef_t(c) = (k - 1)! (n - k)! / n! for t in c and
 *   -k! (n - k - 1)! / n! for t not in c, k = |c|  (the coefficients of a player sum to 0, so the centre changes nothing
 *   but the rounding: the terms are of the size of the effects, not of the ratings).
 *   The accumulation, to the rounding.  The n distinct weights a_k = 1 / (n C(n - 1, k - 1)), k = 1 .. n, are formed in
 *   float64 (the product an exact integer, one division) and rounded to fp32 once; coef_t(c) is a_k for t in c and
 *   -a_(k+1) for t not in c (0 at k = n).  The coalitions are cut into chunks of 1,024 consecutive numbers (one chunk
 *   when n <= 10).  Within a chunk, lane j of 0 .. 15 takes the coalitions c = j (mod 16) in ascending order and chains
 *   s = fma((double)coef_t(c), (double)v(c) - (double)v(2^n - 1), s) in float64 from 0.0 (the difference of two floats
 *   in float64; one rounding per fma); the 16 lane sums are added in float64 by four xor butterflies, s_j + s_(j^1),
 *   then ^2, ^4, ^8.  The chunk sums are chained in float64 in ascending chunk order from 0.0, and the total is rounded
 *   to fp32 once.  A pair's outputs depend on that pair's inputs alone: not on n_p, the grid, P (beyond truncation),
 *   out_values or which pairs share the call.  No float atomics.
 *   out_phi_u [n_p, S_u], out_phi_i [n_p, S_i]  float: phi by slot, +0.0f at every slot that is not a player; either may
 *                    be NULL when its play is NULL
 *   out_base  [n_p] float   v(2^n - 1)       out_empty [n_p] float   v(0)       out_n [n_p] int32   the players played
 *   out_values [n_p, 2^P] float, nullable: entries 0 .. 2^n - 1 hold v(c); the rest are not written
 *   scratch   n_p 2^(P - 10) P doubles when P > 10 (the chunk sums; a second small launch adds them), unused and
 *                    nullable when P <= 10.  Its contents after the call mean nothing.
 *   A pair with n = 0 costs one variant: phi is all zeros and out_base = out_empty.  In a one-side game the other side's
 *   pooled vector is computed once per wave, in a two-side game the item side's once per 2^n_u coalitions.
 *   Limits: 1 <= L <= 64, 1 <= P <= 16, n_u, n_i >= 0, 0 <= n_p < 2^31, with out_values n_p 2^P < 2^31.  Refused before
 *   the launch and the first dereference, in the entry point's own name: a limit; with n_p > 0 a null z, logit, z_pad of
 *   either side, u_idx, i_idx, W1, b1, w, out_base, out_empty or out_n, a null out_phi of a side whose play is given, a
 *   null scratch with P > 10, and n_u or n_i == 0.  n_p == 0 returns R4R_OK and enqueues nothing.  An index outside
 *   [0, n_u) / [0, n_i) is the caller's error.  One launch (two with P > 10); nothing allocates, nothing synchronises.
 * ---------------------------------------------------------------------- */
int r4r_narre_shapley(const float *z_u, const float *logit_u, const float *own_u, const float *z_pad_u, float logit_pad_u,
                      int64_t n_u, int S_u, int R_u,         /* [n_u, S_u, L], [n_u, S_u], [n_u, L] or NULL, [L]      */
                      const float *z_i, const float *logit_i, const float *own_i, const float *z_pad_i, float logit_pad_i,
                      int64_t n_i, int S_i, int R_i,         /* the item side likewise                                */
                      const int64_t *u_idx, const int64_t *i_idx,             /* [n_p] rows of the sides              */
                      const int64_t *start_u, const int64_t *start_i,         /* [n_p] bit masks; NULL = 0            */
                      const int64_t *play_u, const int64_t *play_i,           /* [n_p] bit masks; NULL = 0            */
                      int P, int64_t n_p,                                     /* 1 .. 16                              */
                      const float *q_bias, const float *c_bias,               /* [n_u], [n_i]; NULL = 0               */
                      const float *W1, const float *b1, const float *w, int L,/* [L, L], [L], [L]                     */
                      float *out_phi_u, float *out_phi_i,                     /* [n_p, S_u], [n_p, S_i]; nullable     */
                      float *out_base, float *out_empty, int32_t *out_n,      /* [n_p] each                           */
                      float *out_values,                                      /* [n_p, 2^P], nullable                 */
                      double *scratch,                                        /* n_p 2^(P - 10) P doubles, P > 10     */
                      void *stream);

/* ------------------------------------------------------------------------
 * What-if documents: the single-document families' tower over VARIANTS of an owner's document -- chosen reviews taken
 * away, chosen positions occluded -- from the resident pools (csrc/tower_variants.hip, csrc/docs_masked_device.h).
 * Replaces  the loader's `skip`: a training rating's documents leave the rating's own review out of both sides
 *                                                                       data.py:223-235
 *           pad_and_join / pad_only: cut / zero padded to input_length  data.py:181-210
 *           the documents of a rating outside the training split        data.py:240-246
 *           generalised from ONE removed review to a set, for DeepCoNN, DeepCoNN++ and the TransNets, whose towers read
 *           one document per owner (NARRE's removal re-selects slots and needs no tower: "NARRE what-if scores").
 * The pool (tok, rev_off, first, owners) and ids [n] are those of "Tower spans"; the document layout only (R = 0).
 *
 * r4r_tower_build_variants: ONE launch, one workgroup per row.  Row r, with owner o = ids[r], rb = first[o],
 *   count = first[o + 1] - rb:
 *     kept list   the reviews s in [0, count), ascending, with s >= 64 or bit s of drop[r] clear.  Bits at or beyond count
 *                 are ignored; drop == NULL removes nothing; reviews from the 65th on can never be dropped.
 *     document    docs[r, :] = the tokens of the kept reviews concatenated, the first T of them, padded with word 0.
 *                 With exactly one bit set: data._np_docs(..., skip = that bit, T) integer for integer, the document the
 *                 loader gives a training rating.  With no bit set: r4r_tower_build (R = 0).
 *     occlusion   every position p = occ_pos[j], j in [occ_off[r], occ_off[r + 1]), with 0 <= p < T holds word 0 instead
 *                 (no shift: the padding the model already knows).  Positions outside [0, T) are ignored, repeats are
 *                 harmless.  occ_off == NULL occludes nothing; occ_pos may be NULL only then.  occ_off's entries index
 *                 occ_pos absolutely and need not start at 0: the slice occ_off + a of a longer table serves rows a ..
 *                 with the same occ_pos, without a copy (what the span's rounds pass).
 *     other ids   an id outside [0, owners) gives a zero document; nothing outside the pool is read whatever ids, drop
 *                 or occ_pos hold.
 *   Every element of docs [n, T] is written exactly once.  Refused before the launch and the first dereference, in the
 *   entry point's own name: a null tok, rev_off, first, ids or docs; n outside [0, 2^31); owners < 0; T < 1 or
 *   T > 65536 (the occlusion flags of one row: one bit per position in 8 KB of LDS); occ_off given with a NULL occ_pos.
 *   n == 0 returns R4R_OK and enqueues nothing.
 *
 * r4r_tower_span_variants: r4r_tower_span_fwd at R = 0 with r4r_tower_build_variants in r4r_tower_build's place:
 *   round g covers rows [g group, min(n, (g + 1) group)) and enqueues the builder (drop + g group, occ_off + g group),
 *   r4r_textcnn_fwd over the round's rows and r4r_linear_fwd (no ReLU) into latent + g group L -- the kernels, arguments
 *   and algorithm choice of the per-call entry points, so a span over `group` gives the bits of one
 *   r4r_tower_build_variants + r4r_textcnn_fwd + r4r_linear_fwd call per chunk of `group` rows, and with NULL drop and
 *   occ_off r4r_tower_span_fwd's latents bit for bit.  pooled [n, F] float32 and argmax [n, F] int32 (either nullable):
 *   the rounds' own r4r_textcnn_fwd outputs, copied out of the workspace before the next round overwrites them (what
 *   r4r_textcnn_phrases lists a variant's windows from); asking for them changes no bit of latent.
 *   ws: r4r_tower_span_variants_ws_bytes(group, ...) bytes, r4r_tower_span_fwd's layout.  groups_done (host, out,
 *   nullable): rounds enqueued before an error.  Refusals: r4r_tower_span_fwd's (null pointers, group < 1, E % 4 != 0,
 *   F > 112, a short workspace: R4R_ERR_WORKSPACE) and the builder's, before the first launch.  n == 0 returns R4R_OK and
 *   enqueues nothing.  Nothing allocates, nothing synchronises, no training state is touched.
 * ---------------------------------------------------------------------- */
int r4r_tower_build_variants(const int32_t *tok, const int64_t *rev_off, const int64_t *first, int64_t owners,
                             const int64_t *ids, const int64_t *drop, const int64_t *occ_off, const int32_t *occ_pos,
                             int64_t n, int T, int64_t *docs, void *stream);
size_t r4r_tower_span_variants_ws_bytes(int64_t group, int T, int E, int F, int L, int64_t V);
int r4r_tower_span_variants(const int32_t *tok, const int64_t *rev_off, const int64_t *first, int64_t owners,
                            const int64_t *ids, const int64_t *drop, const int64_t *occ_off, const int32_t *occ_pos,
                            int64_t n, int64_t group, int T, const float *table, int64_t V, const float *conv_w,
                            const float *conv_b, const float *fc_w, const float *fc_b, int E, int F, int L,
                            float *latent, float *pooled, int32_t *argmax, void *ws, size_t ws_bytes,
                            int64_t *groups_done, void *stream);

/* ------------------------------------------------------------------------
 * Document fold: the pooled features of a variant document -- chosen reviews taken away, no occlusion -- without the
 * document and without the tower's gather, and a greedy fewest-review search on top of it (csrc/tower_fold.hip).
 * Replaces  Conv2d + relu + max_pool over a whole document           common_pytorch_models.py:29-31
 *           the document a removal makes: the remaining reviews
 *           joined, cut to input_length, zero padded                data.py:223-235
 *           the frozen word lookup in front of the tower            DeepCoNN.py:53-54
 * With ptab[v, j, f] = sum_k table[v, k] conv_w[f, j, k] a window over the tokens (a, c, d) has the value
 *     y = ((r0 + r1) + r2) + conv_b[f],   r0 = ptab[a, 0, f], r1 = ptab[c, 1, f], r2 = ptab[d, 2, f],
 * a tap outside the document being a row of 0.0f, every add fp32 and in this order.  It depends on the three tokens
 * alone, so the maximum over the windows that lie inside one review (`seg`) is computed once per (owner, review) and a
 * variant row adds only the windows a removal makes new.  pooled[f] = best > 0 ? best : +0.0f, best over all T + 2
 * windows of the variant's document; no -0 appears.  The pool (tok, rev_off, first) and ids are those of "What-if
 * documents"; an id must be an owner of the pool or negative (no reviews), a token a row of ptab: neither can be
 * checked here, the table's height and the pool's size are not arguments.
 *
 * r4r_fold_ptab_stride(F): the floats per word of ptab, PS >= 3 F (0 for F outside 1 .. 112); element (v, j, f) is at
 *   v PS + j F + f.
 * r4r_fold_project: ptab [V, PS] from table [V, E] and conv_w [F, 3, E]: one launch, 64 x 64 tiles, per element one
 *   fmaf chain over k ascending (a float64 sum is within (E + 1) 2^-24 sum_k |x_k w_k| of it).  The pad floats of a
 *   row, 3 F .. PS, are not written.  V == 0 returns R4R_OK and enqueues nothing.
 * r4r_fold_segments: seg [n, S, F].  For owner ids[i] and slot s < min(count, S): the maximum of y over the windows
 *   (r[q - 2], r[q - 1], r[q]), 2 <= q < len, of the owner's s-th review r; -inf where len < 3 and for s >= count.
 *   One wave per (owner, slot): the review's tokens are read 64 at a time, one per lane; then lanes are filters.
 * r4r_fold_compose: pooled [M, F].  Row m with row_owner[m] < 0 is all +0.0f.  Otherwise o = row_owner[m] is an index
 *   into ids and seg, and the row is the pooled features of r4r_tower_build_variants' document of (ids[o], drop[m], no
 *   occlusion, T) -- drop == NULL removes nothing -- by the fold: `pos` = 0 and the last two document tokens (p2, p1)
 *   = (outside, outside); for each kept review r of the first 64 in order and then the run of all reviews from the
 *   65th on as one last run, while pos < T, skipping empty runs, with v = min(len, T - pos):
 *     the windows (p2, p1, r[0]) and, for v >= 2, (p1, r[0], r[1]);
 *     seg[o, s] where v == len and s < S, else the windows (r[q - 2], r[q - 1], r[q]), 2 <= q < v;
 *     (p2, p1) = the last two tokens of the document so far, pos += v;
 *   then min(T - pos, 3) windows that end on the padding's word 0 and the two that hang over the end.  These are all the
 *   distinct windows of the document, so the result equals the maximum over every window, bit for bit.  One wave per
 *   row; a row's bits depend on that row alone: not on M, the order of the rows, or S beyond min(count, 64).
 *
 * The search (the rule of "NARRE counterfactual search" with "attended" replaced by "shows"), one pair per row p of
 * n_p, per searched side a pool, ids, own [n_p] (the pair's index into ids), the current mask [n_p] and S, the slots
 * searched (0 with NULL pointers: the side is not searched); C = S_u + S_i candidate columns, the user side's first:
 * r4r_fold_search_begin: out_scores[p, :] = score0[p], out_order[p, :] = -1, steps = 0, crossed = done = the
 *   comparison (direction 0: score < target, 1: score > target; strict fp32, false for a NaN).
 * r4r_fold_search_rows: a step's candidate rows.  Slot s of a side is a candidate of pair p when p is not done, bit s
 *   is set in cand (NULL: none) and clear in mask, s < min(count, S), the review is not empty and starts before
 *   position T of the CURRENT document (the sum of the kept lengths of the lower slots).  row_owner_u / drop_u [n_p, C]:
 *   column s < S_u holds (own_u[p], mask_u[p] | bit s) for a candidate, else (-1, mask_u[p]); columns >= S_u hold
 *   (-1, mask_u[p]).  row_owner_i / drop_i likewise with the item side's slots in columns S_u + s.
 * r4r_fold_search_pick: the step's winner from cand_score [n_p, C] (one score per candidate row; what a non-candidate
 *   column holds is not read).  The lowest (direction 0) or highest (1) score, ties (float ==) to the lowest column, a
 *   NaN never over a number (all NaN: the lowest column).  A pair that is done is left alone; one without a candidate
 *   becomes done.  Otherwise the winner's bit enters its side's mask, out_order[p, steps] = slot (user side) or
 *   64 + slot (item side), steps += 1, out_scores[p, steps ..] = its score, the winner's latent row n_p + p C + column
 *   of its side's table z [n_p + n_p C, L] is copied to row p (the pair's current latent), crossed = the comparison,
 *   done = crossed or steps == budget.  One wave per pair.
 * Limits: 1 <= F <= 112, E % 4 == 0, 1 <= T <= 65536, 1 <= S <= 64 (0 too for an unsearched side), 1 <= budget <= 64,
 * 1 <= L, rows and pairs < 2^31.  Refused before the launch and the first dereference, in the entry point's own name: a
 * limit and, with work to do, a null pointer.  n == 0 (M, n_p) returns R4R_OK and enqueues nothing.  One launch each;
 * nothing allocates, nothing synchronises.
 * ---------------------------------------------------------------------- */
int r4r_fold_ptab_stride(int F);
int r4r_fold_project(const float *table, int64_t V, const float *conv_w, float *ptab, int E, int F, void *stream);
int r4r_fold_segments(const float *ptab, const float *conv_b, const int32_t *tok, const int64_t *rev_off,
                      const int64_t *first, const int64_t *ids, int64_t n, int S, int F, float *seg, void *stream);
int r4r_fold_compose(const float *ptab, const float *conv_b, const float *seg, int S, const int32_t *tok,
                     const int64_t *rev_off, const int64_t *first, const int64_t *row_owner, const int64_t *ids,
                     const int64_t *drop, int64_t M, int T, int F, float *pooled, void *stream);
int r4r_fold_search_begin(const float *score0, const float *target, int direction, int budget, int64_t n_p,
                          int32_t *out_order, float *out_scores,          /* [n_p, B], [n_p, B + 1]                 */
                          int32_t *out_steps, int32_t *out_crossed, int32_t *done, void *stream);
int r4r_fold_search_rows(const int64_t *rev_off_u, const int64_t *first_u, const int64_t *ids_u, const int64_t *own_u,
                         const int64_t *mask_u, const int64_t *cand_u, int S_u,
                         const int64_t *rev_off_i, const int64_t *first_i, const int64_t *ids_i, const int64_t *own_i,
                         const int64_t *mask_i, const int64_t *cand_i, int S_i,
                         const int32_t *done, int64_t n_p, int T,
                         int64_t *row_owner_u, int64_t *drop_u, int64_t *row_owner_i, int64_t *drop_i, void *stream);
int r4r_fold_search_pick(const float *cand_score, const int64_t *row_owner_u, const int64_t *row_owner_i, int S_u,
                         int S_i, const float *target, int direction, int budget, int64_t n_p, int64_t *mask_u,
                         int64_t *mask_i, float *z_u, float *z_i, int L, int32_t *out_order, float *out_scores,
                         int32_t *out_steps, int32_t *out_crossed, int32_t *done, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* R4R_H */

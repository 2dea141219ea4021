/* libmebt_hip.so — C ABI of the MI355X-native (gfx950) MeBT transformer hot path.
 *
 * This is the drop-in boundary for the path BASELINE.json:north_star names: everything below
 * `mebt.transformer.Net2NetTransformer.forward / reconstruct_mask / shared_step / sample*` and the
 * optimiser step of the reference (Ugness/MeBT) — i.e. what the reference hands to ATen / cuBLAS /
 * NCCL through torch — as hand-written HIP kernels.  Plain pointers and sizes only: no torch types.
 * Every pointer is a DEVICE pointer owned by the caller (PyTorch allocates; the library never
 * allocates device memory: its only scratch — the GEMM tuner's cache-flush buffer and the split-K
 * slabs — is part of the workspace the caller sizes with mebt_workspace_bytes), `stream` is a
 * hipStream_t passed as an opaque pointer (NULL = default stream).  Entry points launch on that
 * stream only and do not synchronise with the host, with ONE exception: in bf16 mode the first
 * launch of a GEMM signature the process has not seen times its tile candidates on the caller's
 * stream (hipEventSynchronize) before it returns.  mebt_gemm_autotune(0), MEBT_GEMM_AUTOTUNE=0, a
 * populated MEBT_GEMM_TUNE_CACHE or a table merged with mebt_gemm_tune_import (the Python host side
 * merges the shipped mebt_amd/tune/gfx950.txt) remove that exception for the signatures they cover;
 * then every entry point is capturable.
 * Re-entrancy: one thread per model handle + workspace; the tuned-configuration table shared by
 * all handles is a mutex-guarded shape -> configuration cache.
 *
 * Each entry point cites the reference code it replaces (paths relative to the reference root).
 * All functions return 0 on success, non-zero on error (MEBT_E*); mebt_last_error() holds a
 * thread-local message (bad shape / unsupported dtype / HIP error string).  The Python host side
 * (mebt_amd/_lib.py) turns a non-zero status into RuntimeError, mirroring the reference's
 * exceptions / asserts.
 */
#ifndef MEBT_HIP_H
#define MEBT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MEBT_ABI_VERSION 2
#define MEBT_MAX_LAYERS 128

typedef void* mebt_stream_t;            /* hipStream_t */
typedef struct mebt_model mebt_model;    /* opaque */

enum mebt_status { MEBT_STATUS_OK = 0, MEBT_STATUS_EINVAL = 1, MEBT_STATUS_ESHAPE = 2, MEBT_STATUS_EHIP = 3,
                   MEBT_STATUS_EWORKSPACE = 4, MEBT_STATUS_EDTYPE = 5 };
enum mebt_dtype { MEBT_DTYPE_F32 = 0, MEBT_DTYPE_BF16 = 1, MEBT_DTYPE_F16 = 2 /* 3D-VQGAN operators only */ };
/* Block routing modes, reference mebt/modules/gpt.py:164-179 */
enum mebt_mode { MEBT_MODE_LATENT_ENC = 0, MEBT_MODE_LATENT_SELF = 1, MEBT_MODE_LATENT_DEC = 2, MEBT_MODE_LT2L = 3,
                 MEBT_MODE_MASKGIT = 4 /* full attention over cat[contexts, targets]: the padding mode of gpt.py:176-178,191-192,208-209 */ };

/* GPT hyper-parameters (reference mebt/modules/gpt.py:200-220, mebt/transformer.py:105-140). */
typedef struct mebt_model_desc {
    int32_t n_layer, n_head, n_embd, vocab, n_latent /* sos_emb */, block_size;
    int32_t dtype;                       /* compute precision: MEBT_DTYPE_BF16 (MFMA bf16, fp32 accumulate) or
                                            MEBT_DTYPE_F32 (exact-fp32 MFMA; the 1e-3 parity mode) */
    int32_t modes[MEBT_MAX_LAYERS];
    float label_smoothing;               /* transformer.py:97-100 */
    float embd_pdrop, resid_pdrop, attn_pdrop;   /* gpt.py:113-114,154,211 */
} mebt_model_desc;

const char* mebt_last_error(void);
int mebt_abi_version(void);

/* ---- model handle ------------------------------------------------------------------------------- */
int mebt_model_create(const mebt_model_desc* desc, mebt_model** out);
void mebt_model_destroy(mebt_model* m);
/* Flat parameter layout.  W = every nn.Linear weight (the decayed AdamW group, transformer.py:769-771),
 * per layer [query,key,value,proj,mlp.0,mlp.2] then head; P = everything else, per layer
 * [ln1.w,ln1.b,ln2.w,ln2.b,query.b,key.b,value.b,proj.b,mlp.0.b,mlp.2.b] then ln_f.w, ln_f.b,
 * mask_emb, sos_emb, pos_emb, tok_emb.  The state-dict tensors of SURVEY.md §A.2 are views into
 * these two buffers. */
int mebt_model_param_counts(const mebt_model* m, int64_t* n_w, int64_t* n_p);
/* W, P: fp32 master parameters; W_lp: bf16 mirror of W (NULL in fp32 mode); gW, gP: fp32 gradient
 * buffers of the same layouts (may be NULL for inference). */
int mebt_model_bind(mebt_model* m, float* W, void* W_lp, float* gW, float* P, float* gP);
/* Refresh the bf16 mirror from the fp32 master weights (after load_state_dict / init). */
int mebt_model_sync_lowp(mebt_model* m, mebt_stream_t stream);
int64_t mebt_workspace_bytes(const mebt_model* m, int32_t B, int32_t NC, int32_t NT, int32_t training);

/* embed + GPT.forward: replaces reference transformer.py:255-283 / :298-322 + gpt.py:234-253.
 * x_ids [B,N] i64 token grid, ci [B,NC] / ti [B,NT] i64 position sets, logits [B,NT,V] fp32 out.
 * training: bit 0 keeps the activations in `ws` for mebt_loss / mebt_backward_*, bit 1 enables
 * dropout (masks keyed by dropout_seed; ignored when all p_drop are 0), bit 2 (inference of a bf16 model only): `logits` points at
 * a bf16 [B,NT,V] buffer and the head stores its fp32 accumulators rounded to bf16 (the sampling loops' draw reads them with
 * mebt_op_sample_lp; the public logits of reconstruct_mask stay fp32). */
int mebt_forward(mebt_model* m, void* ws, int64_t ws_bytes, int32_t B, int32_t N, int32_t NC, int32_t NT,
                 const int64_t* x_ids, const int64_t* ci, const int64_t* ti, float* logits,
                 int32_t training, uint64_t dropout_seed, mebt_stream_t stream);
/* The same forward (inference, bf16 model) for the sampling loops (transformer.py:353-447, :544-663), which call it dozens of times
 * on token grids that differ in a few hundred positions: the key / value projections of the latent_enc blocks — `contexts` is
 * read-only through the network (gpt.py:187-192), so a context position's K / V row depends on its token id, its position and the
 * block's weights only — are kept in a caller-owned cache over ALL N positions, [latent_enc blocks][B][N][2 d] bf16
 * (mebt_kvcache_bytes).  Each call first recomputes the rows of the positions `dirty` [B, ND] (a subset of every sample's `ci`
 * row: embedding, LN1, projection on B * ND rows instead of B * NC) and then reads every block's keys / values at `ci`.  The caller
 * keeps the invariant that a position in `ci` is either in `dirty` or was projected by an earlier call with the token id it still
 * has; the first call of a loop passes dirty = ci.  Same logits as mebt_forward up to the bf16 rounding of a projection tiled for
 * another row count.  flags: 0, or 4 = bf16 logits. */
int64_t mebt_kvcache_bytes(const mebt_model* m, int32_t B, int32_t N);
int mebt_forward_kvcache(mebt_model* m, void* ws, int64_t ws_bytes, int32_t B, int32_t N, int32_t NC, int32_t NT,
                         const int64_t* x_ids, const int64_t* ci, const int64_t* ti, void* logits, int32_t flags,
                         void* kv_cache, const int64_t* dirty, int32_t ND, mebt_stream_t stream);
/* GPT.forward on caller-embedded inputs (reference gpt.py:234-253): sos [B,NS,d], contexts [B,NC,d],
 * targets [B,NT,d] fp32 -> logits [B,NT,V].  Inference (no activations kept); see mebt_gpt_forward_train. */
int mebt_gpt_forward(mebt_model* m, void* ws, int64_t ws_bytes, int32_t B, int32_t NC, int32_t NT, const float* sos,
                     const float* contexts, const float* targets, float* logits, mebt_stream_t stream);
/* The same in training mode: keeps the activations in `ws` for mebt_gpt_backward; dropout != 0 enables the
 * embd / attn / resid dropout sites of gpt.py:135,140,154,238-240 under `dropout_seed`. */
int mebt_gpt_forward_train(mebt_model* m, void* ws, int64_t ws_bytes, int32_t B, int32_t NC, int32_t NT, const float* sos,
                           const float* contexts, const float* targets, float* logits, int32_t dropout, uint64_t dropout_seed,
                           mebt_stream_t stream);
/* Backward of GPT.forward (the autograd backward of gpt.py:234-253) from dL/dlogits [B,NT,V] fp32 after
 * mebt_gpt_forward_train: block / ln_f / head parameter gradients into gW, gP (the embedding slices of gP are left zero) and the
 * gradients of the three embedded inputs, fp32 like the inputs (each may be NULL).  Inputs the logits do not depend on
 * get zeros. */
int mebt_gpt_backward(mebt_model* m, void* ws, const float* dlogits, float* d_sos, float* d_contexts, float* d_targets,
                      mebt_stream_t stream);
/* Masked-token loss + top-1/top-5 of the last mebt_forward: replaces F.cross_entropy(sum,
 * label_smoothing) and utils.accuracy (transformer.py:726-731, utils.py:80-94).
 * out4 (device, 4 doubles) = { CE sum, #top-1 hits, #top-5 hits, #rows }. */
int mebt_loss(mebt_model* m, void* ws, const float* logits, double* out4, mebt_stream_t stream);
/* The same, and additionally the gradient of (CE sum * loss_scale) with respect to the logits from the same pass over them (kept
 * in the workspace): a following mebt_backward_head with the same loss_scale and no upstream skips its cross-entropy backward
 * (F.cross_entropy forward + backward of transformer.py:726 in one read of the logits).  Vocabulary sizes the fused kernel does
 * not cover behave like mebt_loss. */
int mebt_loss_with_grad(mebt_model* m, void* ws, const float* logits, double* out4, float loss_scale, mebt_stream_t stream);
/* Backward of loss = CE_sum * loss_scale (* *upstream if non-NULL, a device scalar), split so the
 * caller can overlap the data-parallel all-reduce of finished gradient buckets with the rest
 * (reference: DDP reducer, train_transformer.py:39-41).  Order: head, layers hi..lo descending, embed. */
int mebt_backward_head(mebt_model* m, void* ws, const float* logits, const float* upstream, float loss_scale, mebt_stream_t stream);
/* Same, from an explicit upstream gradient dL/dlogits [B,NT,V] fp32 (caller-computed loss). */
int mebt_backward_head_dlogits(mebt_model* m, void* ws, const float* dlogits, mebt_stream_t stream);
int mebt_backward_layers(mebt_model* m, void* ws, int32_t layer_hi, int32_t layer_lo, mebt_stream_t stream);
int mebt_backward_embed(mebt_model* m, void* ws, mebt_stream_t stream);
/* Fused AdamW over both flat buffers + refresh of the bf16 mirror: replaces torch.optim.AdamW with
 * the 4 groups of transformer.py:790-797 (W decayed, P not).  step >= 1; grad_scale multiplies the
 * gradients (1/world_size when the all-reduce summed). Parameters the loss cannot reach (blocks
 * after the last latent_dec) are skipped like torch skips grad=None. */
int mebt_adamw_step(mebt_model* m, float* mW, float* vW, float* mP, float* vP, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int32_t step, float grad_scale, mebt_stream_t stream);

/* The same update restricted to one gradient bucket — kind 0: head weight; 1: blocks layer_lo..layer_hi;
 * 2: the P tail (ln_f + embeddings); 3: everything; 4: everything except the blocks' Linear weights (after a
 * backward with the fused optimizer armed).  Buckets are disjoint: a caller may issue each on its
 * own stream as soon as that bucket's gradients are final (after its all-reduce), overlapping the HBM-bound
 * optimizer with the rest of backward. */
int mebt_adamw_range(mebt_model* m, float* mW, float* vW, float* mP, float* vP, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int32_t step, float grad_scale, int32_t kind, int32_t layer_hi,
                     int32_t layer_lo, mebt_stream_t stream);

/* The same update on an arbitrary slice [off, off + n) of W (which = 0) or P (which = 1) with the gradient passed
 * separately (`grad` = gradient of element `off`; bf16 when grad_bf16): what a data-parallel rank applies to its shard
 * of a gradient bucket after the reduce-scatter — optimizer state and fp32 masters are only touched by the owner
 * (reference: the DDP all-reduce + replicated optimizer of train_transformer.py:39-41). */
int mebt_adamw_slice(mebt_model* m, int32_t which, int64_t off, int64_t n, const void* grad, int32_t grad_bf16, float* mW,
                     float* vW, float* mP, float* vP, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int32_t step, float grad_scale, mebt_stream_t stream);

/* The same update with the slice's gradient given as `pieces` bf16 copies of it, piece j at grad_pieces + j * n elements: rank j's
 * contribution to this rank's shard as an all-to-all delivers them.  The kernel adds the pieces in fp32, in piece order, then
 * applies AdamW to the sum: 2 B per parameter on the wire like a bf16 reduce-scatter, but the cross-rank sum is taken in fp32 as
 * the reference's DDP all-reduce takes it (train_transformer.py:39-41) instead of in bf16 inside RCCL. */
int mebt_adamw_slice_pieces(mebt_model* m, int32_t which, int64_t off, int64_t n, const void* grad_pieces, int32_t pieces, float* mW,
                            float* vW, float* mP, float* vP, float lr, float beta1, float beta2, float eps, float weight_decay,
                            int32_t step, float grad_scale, mebt_stream_t stream);

/* Optimizer-in-backward (single-process training): armed with step >= 1, the next mebt_backward_layers applies
 * AdamW to every block's Linear weights INSIDE the weight-gradient launch (the gradient tile is consumed from
 * registers; it is not stored in gW, and W / the bf16 mirror / mW / vW are updated in place), which removes
 * 8 of the 34 bytes per parameter the separate optimizer pass moves and hides the rest behind the MFMA work.
 * The remaining parameters are then updated with mebt_adamw_range(kind = 4).  step <= 0 disarms.  Same math as
 * mebt_adamw_step (torch.optim.AdamW, transformer.py:790-797); not usable when gradients must be all-reduced
 * or inspected first. */
int mebt_model_set_fused_adamw(mebt_model* m, float* mW, float* vW, float lr, float beta1, float beta2, float eps,
                               float weight_decay, int32_t step, float grad_scale);

/* Data-parallel wire format: gWb = bf16 buffer of n_w elements laid out like gW (NULL: off).  While bound (bf16 compute mode, no
 * gradient accumulation, fused optimizer disarmed) mebt_backward_* store the Linear weight gradients THERE, rounded once from
 * the fp32 MFMA accumulators, and leave gW untouched: the reduce-scatter of SURVEY.md §5.8 sends the buffer as is. */
int mebt_model_bind_wire_grads(mebt_model* m, void* gWb);

/* Sharded data parallelism (mebt_amd/parallel.py; the reference's counterpart is DDP's all-reduce, train_transformer.py:39-41):
 * the all-gathers that bring the other ranks' updated parameters may still be running when the next forward is enqueued.
 * `events[i]` (a hipEvent_t the caller recorded after the gather) must have completed before the forward touches the
 * parameters first read by block `layer[i]`; layer -1 = everything outside the Linear weights (embeddings, biases,
 * LayerNorms: read from the first kernel on), layer n_layer = the head weight.  One-shot: the next forward on this
 * model (training or inference) waits for them on its stream (hipStreamWaitEvent, no host synchronisation) and forgets
 * them.  The events stay owned by the caller and must outlive that forward's enqueue. */
int mebt_model_set_forward_waits(mebt_model* m, int32_t n, const int32_t* layer, void* const* events);
/* Gradient accumulation over micro-batches (reference train_transformer.py:46-49, Lightning's accumulate_grad_batches):
 * on = 1: the following mebt_backward_* calls ADD to gW / gP; on = 0 (default): they overwrite.  Not together with
 * mebt_model_set_fused_adamw. */
int mebt_model_set_grad_accumulate(mebt_model* m, int32_t on);

/* ---- operator entry points (building blocks; also what the parity tests call) ---------------------- */
/* C[M,N] = sum_k A(m,k) B(n,k) + bias, epilogue 0 none / 1 GELU (C=pre, C2=gelu) / 2 +aux residual /
 * 3 * gelu'(aux).  a_kc/b_kc: 1 = operand stored [rows][K], 0 = stored [K][rows].  Replaces nn.Linear
 * forward / dgrad / wgrad (gpt.py:126-128,140,150-155,248). */
int mebt_op_gemm(int32_t dtype, const void* A, const void* B, void* C, void* C2, const float* bias, const void* aux,
                 int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldb, int32_t ldc, int32_t ld_aux,
                 int32_t a_kc, int32_t b_kc, int32_t epilogue, int32_t c_f32, int32_t beta, int32_t split_k,
                 mebt_stream_t stream);
/* nn.LayerNorm(d), eps 1e-5 (gpt.py:147-148,216). */
int mebt_op_layernorm_fwd(int32_t dtype, const void* x, void* y, const float* gamma, const float* beta, float* mean,
                          float* rstd, int32_t rows, int32_t d, mebt_stream_t stream);
int mebt_op_layernorm_bwd(int32_t dtype, const void* x, const void* dy, const float* gamma, const float* mean,
                          const float* rstd, void* dx, float* dgamma, float* dbeta, int32_t rows, int32_t d,
                          mebt_stream_t stream);
/* softmax(q k^T / sqrt(hd)) v (gpt.py:131-137).  q [B,NQ,H,hd] row stride ldq etc.; lse [B,H,NQ]. */
int mebt_op_attention_fwd(int32_t dtype, const void* q, const void* k, const void* v, void* o, float* lse, int32_t B,
                          int32_t H, int32_t NQ, int32_t NK, int32_t HD, int32_t ldq, int32_t ldk, int32_t ldv,
                          int32_t ldo, int32_t force_generic, mebt_stream_t stream);
/* Tests only: the same forward with gathered keys / values, as the sampling loops' cache is read: key / value row r of sample b is row
 * kidx[b * NK + r] of a buffer of `kidx_rows` rows per sample (k, v point at sample 0, row 0).  bf16 MFMA forward only, NK <= 8192;
 * anything else (fp32, force_generic, another head size) is MEBT_STATUS_ESHAPE. */
int mebt_op_attention_fwd_gather(int32_t dtype, const void* q, const void* k, const void* v, void* o, float* lse, int32_t B,
                                 int32_t H, int32_t NQ, int32_t NK, int32_t HD, int32_t ldq, int32_t ldk, int32_t ldv,
                                 int32_t ldo, int32_t force_generic, const int32_t* kidx, int32_t kidx_rows, mebt_stream_t stream);
int mebt_op_attention_bwd(int32_t dtype, const void* q, const void* k, const void* v, const void* o, const float* lse,
                          const void* d_o, void* dq, void* dk, void* dv, float* delta, int32_t B, int32_t H,
                          int32_t NQ, int32_t NK, int32_t HD, int32_t ldq, int32_t ldk, int32_t ldv, int32_t ldo,
                          int32_t force_generic, mebt_stream_t stream);
/* Embedding gather (transformer.py:255-277): sos/ctx/tgt [B,*,d] of element type `dtype`. */
int mebt_op_embed_fwd(int32_t dtype, const int64_t* x_ids, const int64_t* ci, const int64_t* ti, const float* tok_emb,
                      const float* pos_emb, const float* mask_emb, const float* sos_emb, void* sos, void* ctx, void* tgt,
                      int32_t B, int32_t N, int32_t NC, int32_t NT, int32_t NS, int32_t d, int32_t vocab,
                      int32_t block_size, mebt_stream_t stream);
/* Categorical draw of sample_from_logits / gumbel_sort (transformer.py:826-910) with the Exp(1) noise
 * as an explicit input: ids = argmax(p/noise), score = p[ids]; probs optional [rows,V]. */
int mebt_op_sample(const float* logits, const float* noise, float temperature, int32_t top_k, float top_p, int64_t* ids,
                   float* score, float* probs, int32_t rows, int32_t V, mebt_stream_t stream);
/* The same with q drawn INSIDE the kernel from a counter-based generator (element (row, e) of the step keyed by `seed`; CPU twin
 * oracle/closed_form.py:exp1_counter): only the logits move through HBM.  The explicit-noise entry above stays the bit-exact
 * interface for golden tests. */
int mebt_op_sample_seeded(const float* logits, uint64_t seed, float temperature, int32_t top_k, float top_p, int64_t* ids,
                          float* score, float* probs, int32_t rows, int32_t V, mebt_stream_t stream);
/* The weight gradients of one block in ONE launch (the autograd backward of nn.Linear weights and biases, gpt.py:126-128,140,150-155):
 * item i: dW_i[n_out_i, k_in_i] = dY_i^T X_i over tokens_i rows (bf16 row-major operands) -> gW + w_off[i] (fp32); bias[i] (or NULL)
 * += column sums of dY_i (atomic adds: zero it first).  fused != 0 applies AdamW in place of the store (optimizer-in-backward,
 * transformer.py:665-681,790-797): W, mW, vW (+ bf16 mirror Wlp, may be NULL) at the same offsets.  n <= 8. */
int mebt_op_wgrad_grouped(int32_t n, const void* const* dY, const void* const* X, const int32_t* n_out, const int32_t* k_in,
                          const int32_t* tokens, const int64_t* w_off, float* const* bias, float* W, float* gW, float* mW, float* vW,
                          void* Wlp, int32_t fused, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                          float grad_scale, mebt_stream_t stream);
/* Tests: two independent bf16 products in ONE launch, as the engine issues the q and k|v projections of a block (forward and dgrad).
 * Every per-product argument is an array of two: C_i[M_i, N_i] = A_i B_i^T + bias_i, A_i stored [M_i][K_i] (row stride lda_i), B_i stored
 * [N_i][K_i] (b_kc = 1) or [K_i][N_i] (b_kc = 0, both products alike), epilogue_i 0 none / 2 + aux_i residual / 3 * gelu'(aux_i) (there is no
 * C2, so no GELU), c_f32_i != 0: fp32 C_i.  bias / aux may be NULL or hold NULLs.  One pair kernel runs when both outputs are bf16, every
 * K_i is a multiple of 64, every N_i a multiple of 8 and no single-product tile / variant is forced; otherwise the products go out as
 * two ordinary launches under the rules of mebt_op_gemm.  Null operands and bad epilogues are MEBT_STATUS_EINVAL, bad extents
 * MEBT_STATUS_ESHAPE, before anything is launched. */
int mebt_op_gemm_pair(const void* const* A, const void* const* B, void* const* C, const float* const* bias, const void* const* aux,
                      const int32_t* M, const int32_t* N, const int32_t* K, const int32_t* lda, const int32_t* ldb, const int32_t* ldc,
                      const int32_t* ld_aux, const int32_t* epilogue, const int32_t* c_f32, int32_t b_kc, mebt_stream_t stream);
/* kth[r] = the top_k-th largest value of row r of logits [rows, V] (1 <= top_k < V): the threshold of the reference's module-level
 * `top_k_logits` (transformer.py:891-895: everything below it becomes -inf, ties are kept).  ids_scratch: [rows] int64. */
int mebt_op_topk_threshold(const float* logits, int32_t top_k, float* kth, int64_t* ids_scratch, int32_t rows, int32_t V,
                           mebt_stream_t stream);
/* x[b, ti[b,j]] = ids[b,j]  (the sparse_coo/to_dense/where scatter of transformer.py:413-439). */
/* sample(debug=True) (transformer.py:395,426-436): the same draw for rows = B * NT target positions, each row's probabilities
 * written straight to row ti[b, j] of the [B, N, V] probability map (the reference materialises [B, NT, V] and scatter_()s it).
 * noise = NULL: Exp(1) drawn in the kernel from `seed`.  V = 16384, no top-p. */
int mebt_op_sample_scatter(const float* logits, const float* noise, uint64_t seed, float temperature, int32_t top_k, int64_t* ids,
                           float* score, float* probs_map, const int64_t* ti, int32_t B, int32_t N, int32_t NT, int32_t V,
                           mebt_stream_t stream);
/* The same draw on the logits as the head of an in-engine sampling loop wrote them: fp32 (logits_bf16 = 0) or bf16 (1: mebt_forward
 * with flag 4 — half the bytes of the [rows, V] tensor on both sides).  rows = B * NT; noise = NULL: Exp(1) drawn in the kernel from
 * `seed`; probs_map + ti (both or neither): the debug=True probability map as in mebt_op_sample_scatter.  V = 16384, no top-p.
 * draw: 0 = arg-max p / q with q ~ Exp(1) per element (the reference's arithmetic, transformer.py:826-841: bit-exact ids for an
 * injected `noise`); 1 (noise = NULL only) = inverse CDF from ONE uniform per row keyed by (seed, row) — a sample of the same
 * categorical distribution p (what the reference's draw is) without the per-element hash, logarithm and reciprocal: the production
 * draw of the sampling loops. */
int mebt_op_sample_lp(const void* logits, int32_t logits_bf16, const float* noise, uint64_t seed, float temperature, int32_t top_k,
                      int64_t* ids, float* score, float* probs_map, const int64_t* ti, int32_t B, int32_t N, int32_t NT, int32_t V,
                      int32_t draw, mebt_stream_t stream);
int mebt_op_scatter_ids(int64_t* x, const int64_t* ti, const int64_t* ids, int32_t B, int32_t N, int32_t NT,
                        mebt_stream_t stream);
/* MaskGen.generate_next_mask + gumbel_top_k (mask_sampler.py:178-246): order targets by
 * (score/sum)/noise^ctemp descending; first n_new go to the context (appended), the rest stay
 * targets in score order. */
int mebt_op_next_mask(const int64_t* ci, const int64_t* ti, const float* score, const float* noise, float ctemp,
                      int32_t n_new, int32_t B, int32_t NC, int32_t NT, int64_t* new_ci, int64_t* new_ti,
                      mebt_stream_t stream);
/* fp32 -> bf16 cast of a flat buffer (n multiple of 4). */
int mebt_op_cast_bf16(const float* src, void* dst, int64_t n, mebt_stream_t stream);

/* ---- the row kernels in every form the engine launches (what tests/test_gpu_row_ops.py calls) ------
 * Thin marshalling onto the launchers of the train step.  Every refusal (null required pointer, bad dtype, a width that is no
 * multiple of 4, too many jobs) is decided on the host before anything is launched; empty shapes return 0 and launch nothing. */
#define MEBT_LN_MAX_JOBS 3
/* One LayerNorm of a multi-job launch.  Row r of `x` belongs to row map(r) = (r / seg) * seg_stride + seg_off + r % seg of the
 * mapped tensors (seg = 0: identity).  Forward: y, mean, rstd are written at the mapped row (mean = rstd = NULL: inference form).
 * Backward: dy, mean, rstd are read at the mapped row, x / dy2 / dx_add / dx / dx2 at the plain row, and
 *   dx = LN'(dy + dy2) + (dx_add + old dx)      (dy2, dx_add optional; old dx only with dx_accumulate)
 * dx_f32 = 1: dx / dx2 are fp32 although the job is bf16.  dx2 (optional) = stored dx * the keep-scale of dropout site
 * (drop_seed, drop_site, drop_p) at element row * d + e, as mebt_debug_dropout_mask returns it; drop_p = 0: no mask.
 * dgamma / dbeta (fp32) are added to.  Jobs with rows <= 0 are skipped and do not count towards MEBT_LN_MAX_JOBS. */
typedef struct mebt_ln_job {
    const void* x;
    void* y;
    const void* dy;
    const void* dy2;
    const void* dx_add;
    const float* gamma;
    const float* beta;
    float* mean;
    float* rstd;
    void* dx;
    void* dx2;
    float* dgamma;
    float* dbeta;
    int32_t rows, d, seg, seg_stride, seg_off;
    int32_t dx_f32, dx_accumulate;
    uint32_t drop_site;
    uint64_t drop_seed;
    float drop_p;
    int32_t reserved;
} mebt_ln_job;
/* out[n] += sum_m X[m, n]: X [M, N] of `dtype` at row pitch ldx (elements, a multiple of 4), N a multiple of 4, out fp32 */
typedef struct mebt_colsum_item {
    const void* X;
    float* out;
    int32_t M, N, ldx;
    int32_t reserved;
} mebt_colsum_item;
int mebt_op_layernorm_fwd_jobs(int32_t dtype, const mebt_ln_job* jobs, int32_t n, mebt_stream_t stream);
/* n_colsums > 0: these column sums (at most 12) are computed by extra workgroups of the same launch */
int mebt_op_layernorm_bwd_jobs(int32_t dtype, const mebt_ln_job* jobs, int32_t n, const mebt_colsum_item* colsums, int32_t n_colsums,
                               mebt_stream_t stream);
int mebt_op_colsum(int32_t dtype, const void* X, int32_t M, int32_t N, int32_t ldx, float* out, mebt_stream_t stream);
int mebt_op_colsum_grouped(int32_t dtype, const mebt_colsum_item* items, int32_t n, mebt_stream_t stream);
/* The masked-token loss of rows = B * NT logit rows [rows, V] fp32 (V a multiple of 4); the target of row (b, j) is
 * x_ids[b, ti[b, j]].  Per row: row_lse, row_loss (label-smoothed), row_rank (classes ranked above the target; among equal logits
 * the lower index ranks higher); out4 (double): loss sum, top-1 count, top-5 count, rows.  dlogits (optional, fp32 or bf16 by
 * dl_bf16) = d(loss sum * grad_scale) / dlogits from the same pass: V = 16384 only, left untouched at every other V. */
int mebt_op_cross_entropy(const float* logits, const int64_t* x_ids, const int64_t* ti, int32_t B, int32_t N, int32_t NT, int32_t V,
                          float label_smoothing, float* row_lse, float* row_loss, int32_t* row_rank, double* out4, void* dlogits,
                          int32_t dl_bf16, float grad_scale, mebt_stream_t stream);
/* dlogits [rows, V] of `dtype` = (softmax - smoothed one-hot) * scale * (*upstream, a device scalar, or 1 when NULL) */
int mebt_op_cross_entropy_bwd(int32_t dtype, const float* logits, const int64_t* x_ids, const int64_t* ti, const float* row_lse,
                              const float* upstream, float scale, float label_smoothing, void* dlogits, int32_t B, int32_t N,
                              int32_t NT, int32_t V, mebt_stream_t stream);
/* AdamW (torch.optim.AdamW semantics) over a flat buffer of n elements (a multiple of 4), step >= 1; p_bf16 (optional): bf16 mirror of
 * the updated p.  g is fp32, or (g_bf16) the fp32 sum of g_pieces bf16 copies, copy j at g + j * g_stride elements. */
int mebt_op_adamw(float* p, const void* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, float grad_scale, int32_t g_bf16, int32_t g_pieces, int64_t g_stride,
                  mebt_stream_t stream);
/* Backward of mebt_op_embed_fwd: g_ctx [B, NC, d] fp32, g_tgt [B, NT, d] and g_sos [B, NS, d] of `dtype` are added into the fp32
 * gradients of tok_emb / pos_emb (by token and position), mask_emb (all target rows) and sos_emb (over the batch). */
int mebt_op_embed_bwd(int32_t dtype, const int64_t* x_ids, const int64_t* ci, const int64_t* ti, const float* g_ctx, const void* g_tgt,
                      const void* g_sos, float* g_tok_emb, float* g_pos_emb, float* g_mask_emb, float* g_sos_emb, int32_t B, int32_t N,
                      int32_t NC, int32_t NT, int32_t NS, int32_t d, mebt_stream_t stream);
/* dst[map_d(r)] = src[map_s(r)] for r < rows, rows of d elements (a multiple of 4), fp32 or bf16 on either side (bf16 stores round
 * to nearest even); map(r) = (r / seg) * stride + off + r % seg, seg = 0: identity */
int mebt_op_copy_rows(const void* src, void* dst, int64_t rows, int32_t d, int32_t src_f32, int32_t dst_f32, int32_t s_seg,
                      int32_t s_stride, int32_t s_off, int32_t d_seg, int32_t d_stride, int32_t d_off, mebt_stream_t stream);
/* rows of row_bytes bytes (a multiple of 16) moved by idx [B, n]: gather dst[b * n + j] = src[b * npos + idx[b, j]], scatter the
 * inverse; positions outside [0, npos) are skipped */
int mebt_op_index_rows(const void* src, void* dst, const int64_t* idx, int32_t B, int32_t n, int32_t npos, int32_t row_bytes,
                       int32_t scatter, mebt_stream_t stream);

/* 0: never time GEMM candidates (measured heuristic or cached choices only: no host synchronisation anywhere);
 * 1: tune unseen signatures at their first launch (default; environment MEBT_GEMM_AUTOTUNE). */
void mebt_gemm_autotune(int32_t mode);
int32_t mebt_gemm_autotune_enabled(void);      /* the current mode */
/* The tuned-configuration table as text (one `n k_0 .. k_{n-1} value` entry per line + a version entry): export returns the bytes
 * needed incl. the terminating 0 and writes them when `cap` suffices; import merges a text (overwrite = 1: its entries replace the
 * ones this process holds; 2: the table is dropped first, i.e. replaced; 0: they only fill gaps) and returns the number of entries taken (0 for a text written by a build
 * with other variant codes).  A data-parallel job broadcasts rank 0's table after its first step so that every rank launches
 * identical kernels (reference train_transformer.py:39-46: DDP replicas run the same program); mebt_amd ships a default table
 * (mebt_amd/tune/gfx950.txt) merged with overwrite = 0 at load time, so a fresh process does not stall on in-situ tuning. */
int64_t mebt_gemm_tune_export(char* buf, int64_t cap);
int32_t mebt_gemm_tune_import(const char* text, int32_t overwrite);
/* diagnostics: the fastest few candidates (value, isolated microseconds) of every signature this process tuned, one line each
 * (`n k.. : v us v us ...`); tools/step_tune.py tries them inside the train step.  Same size protocol as mebt_gemm_tune_export. */
int64_t mebt_gemm_tune_alternatives(char* buf, int64_t cap);

/* ---- 3D-VQGAN first stage (reference mebt/vqgan.py:82-93,255-424, modules/codebook.py:52-62) ------------
 * Activations are channels-last [B, T, H, W, C] of `dtype` (MEBT_DTYPE_F16: MFMA fast mode, MEBT_DTYPE_F32: parity mode); the
 * video at the network boundary stays the reference's fp32 [B, C, T, H, W]. */
#define MEBT_CONV_MAX_TAPS 64
/* One (sub-lattice) convolution as an implicit GEMM.  Output voxel o = o' * os + pi for o' < (cT, cH, cW) reads, for tap j, the
 * input voxel clamp(o' * sm + tap[j]) (replicate padding, SamePadConv3d vqgan.py:374-398).  A stride-2 transposed convolution
 * (SamePadConvTranspose3d :401-424) is issued once per output parity class with the taps of that class.  w: [Cout][ntaps][Cin]
 * of `dtype`; bias fp32 [Cout] or NULL; resid (optional) is added to the result (ResBlock x + h, :370), laid out like `out`. */
typedef struct mebt_conv3d_desc {
    const void* in; void* out; const void* w; const float* bias; const void* resid;
    int32_t B, Ti, Hi, Wi, Cin, To, Ho, Wo, Cout;
    int32_t cT, cH, cW;
    int32_t os[3], pi[3], sm[3];
    int32_t ntaps;
    int8_t tap[MEBT_CONV_MAX_TAPS][4];
    int32_t in_mode;    /* 0: channels-last `dtype`; 1: fp32 [B, C, T, H, W] */
    int32_t out_mode;   /* 0: channels-last `dtype`; 1: channels-last fp32; 2: fp32 [B, C, T, H, W] */
} mebt_conv3d_desc;
/* allow_mfma = 0 forces the direct fp32-FMA kernel (the on-GPU reference of the MFMA kernel). */
int mebt_op_conv3d(int32_t dtype, const mebt_conv3d_desc* d, int32_t allow_mfma, mebt_stream_t stream);
/* The kernel mebt_op_conv3d runs for this descriptor, as a stable name: "dma_<bm>x<bn>x<ring>" (LDS-DMA implicit GEMM), "mfma_f16"
 * (register-staged), "first_mfma", "last_mfma_<Cin / 32>", "voxel_<4|32>", "direct"; "none" for an empty class, NULL (error text set)
 * for what mebt_op_conv3d refuses.  Host only: no GPU call, and only the descriptor's integers and whether `resid` is set are read. */
const char* mebt_conv3d_route(int32_t dtype, const mebt_conv3d_desc* d, int32_t allow_mfma);
/* y = silu(GroupNorm_32(x)), eps 1e-6 (vqgan.py:255-258,17-18); stats: scratch [B, 32, 2] fp32. */
int mebt_op_groupnorm_silu(int32_t dtype, const void* x, void* y, const float* gamma, const float* beta, float* stats, int32_t B,
                           int64_t vox_per_sample, int32_t C, mebt_stream_t stream);
/* ids[m] = argmin_j |z_m - e_j|^2 in the reference's evaluation order (codebook.py:54-58); z fp32 [M, d], embeddings fp32
 * [n_codes, d]; score (scratch [M, n_codes] fp32) receives z E^T from the exact-fp32 MFMA GEMM, esq scratch [n_codes]. */
int mebt_op_codebook_argmin(const float* z, const float* embeddings, float* score, float* esq, int64_t* ids, int32_t M,
                            int32_t n_codes, int32_t d, mebt_stream_t stream);
/* The same ids through a filtered search: approximate scores on the bf16 MFMA GEMM (stored as bf16), then the exact fp32 distance of
 * every code that can still be the arg-min given the rounding bound (never a reduced-precision decision).  score: scratch of at
 * least M * n_codes * 2 bytes (the exact search's fp32 matrix qualifies); lowp: scratch of (M + n_codes) * d bf16 values; esq:
 * scratch [n_codes + 1]; embedding_dim a multiple of 64. */
int mebt_op_codebook_argmin_filtered(const float* z, const float* embeddings, void* score, float* esq, void* lowp, int64_t* ids,
                                     int32_t M, int32_t n_codes, int32_t d, mebt_stream_t stream);
/* out[m, :] = embeddings[ids[m], :] (F.embedding of VQGAN.decode, vqgan.py:91), out of `dtype`. */
int mebt_op_embedding_rows(int32_t dtype, const int64_t* ids, const float* embeddings, void* out, int64_t rows, int32_t d,
                           int32_t n_codes, mebt_stream_t stream);
/* fp32 -> fp16 cast of a flat buffer (n multiple of 4). */
int mebt_op_cast_f16(const float* src, void* dst, int64_t n, mebt_stream_t stream);

/* ---- 3D-VQGAN first stage, backward (csrc/vqgan_bwd/vqgan_bwd.hip; reference mebt/vqgan.py:98-102,183-184 before discriminator_iter_start) -----
 * Same conventions as above.  Every floating-point sum over workgroups is a fixed-order sum of fp32 partial slabs in caller-sized
 * scratch (no float atomics, no hand-off inside a launch): the same inputs give the same bits.  `inv_scale` (1 / S of a backward pass
 * seeded with the power-of-two gradient scale S) multiplies the parameter gradients in the fp32 epilogue.
 *
 * Data gradient of one mebt_conv3d_desc class: the gradient on the PADDED input lattice (q = clamp-free coordinate + front) is a
 * convolution of dy that reads zeros outside dy; mebt_op_pad_zero makes the zero border physical so that mebt_op_conv3d computes it
 * (out_mode 1, fp32), and mebt_op_halo_fold adds every lattice position onto the voxel the forward's clamp mapped it to.
 * mebt_op_pad_zero: dst [B, pT, pH, pW, C] of `dtype`, channels-last = src placed at (fT, fH, fW), zero elsewhere; src [B, T, H, W, C]
 * of `dtype` (src_mode 0) or fp32 (1), or fp32 [B, C, T, H, W] (2).  p >= n + f per dimension, else MEBT_STATUS_ESHAPE. */
int mebt_op_pad_zero(int32_t dtype, const void* src, void* dst, int32_t B, int32_t T, int32_t H, int32_t W, int32_t fT, int32_t fH,
                     int32_t fW, int32_t pT, int32_t pH, int32_t pW, int32_t C, int32_t src_mode, mebt_stream_t stream);
/* dx[b, i, c] = add[b, i, c] + sum of dxp[b, q, c] over the lattice positions q (fp32 [B, pT, pH, pW, C]) with clamp(q - f, 0, n - 1) == i
 * per dimension: q = i + f inside, the first voxel also takes q < f, the last one q >= n + f, a one-voxel axis all of them.  add
 * (channels-last `dtype`, the residual branch's gradient) may be NULL.  dx: channels-last `dtype` (out_mode 0) or fp32 (1). */
int mebt_op_halo_fold(int32_t dtype, const float* dxp, const void* add, void* dx, int32_t B, int32_t T, int32_t H, int32_t W, int32_t pT,
                      int32_t pH, int32_t pW, int32_t fT, int32_t fH, int32_t fW, int32_t C, int32_t out_mode, mebt_stream_t stream);
/* Weight and bias gradient of one class: dw[co][j][ci] = inv_scale * sum_o dy[o][co] x[clamp(o' sm + tap[j])][ci] (fp32, the class layout
 * [Cout][ntaps][Cin]) and db[co] = inv_scale * sum_o dy[o][co] (NULL: not wanted).  The descriptor is the forward's: `in` = x (in_mode 0
 * or 1), `out` = dy in the layout of out_mode (0, 1 or 2; read only), `w`, `bias`, `resid` unused.  fp16: v_mfma_f32_16x16x32_f16 on
 * operands rounded to fp16; fp32: FMAs.  The voxels are split over at most `nsplit` workgroups per tile; scratch holds
 * mebt_conv3d_wgrad_scratch_bytes(d, nsplit) bytes.  An empty class writes zeros. */
int64_t mebt_conv3d_wgrad_scratch_bytes(const mebt_conv3d_desc* d, int32_t nsplit);
int mebt_op_conv3d_wgrad(int32_t dtype, const mebt_conv3d_desc* d, float* dw, float* db, float inv_scale, int32_t nsplit, void* scratch,
                         int64_t scratch_bytes, mebt_stream_t stream);
/* Backward of y = silu(GroupNorm_32(x)): with xhat, h = xhat gamma + beta and s = sigmoid(h) recomputed from x and the forward's `stats`,
 * dh = dy s (1 + h (1 - s)); dgamma_c = inv_scale * sum dh xhat, dbeta_c = inv_scale * sum dh; dx = rstd (gamma dh - mean_g(gamma dh) -
 * xhat mean_g(gamma dh xhat)) + add (add: channels-last `dtype` or NULL).  x, dy, dx channels-last `dtype`.  scratch (8-byte aligned):
 * mebt_groupnorm_silu_bwd_scratch_bytes(B, vox_per_sample, C) bytes. */
int64_t mebt_groupnorm_silu_bwd_scratch_bytes(int32_t B, int64_t vox_per_sample, int32_t C);
int mebt_op_groupnorm_silu_bwd(int32_t dtype, const void* x, const float* stats, const float* gamma, const float* beta, const void* dy,
                               const void* add, void* dx, float* dgamma, float* dbeta, float inv_scale, int32_t B,
                               int64_t vox_per_sample, int32_t C, void* scratch, int64_t scratch_bytes, mebt_stream_t stream);
/* out[i] = c * sign(x_recon[i] - x[i]) with sign(0) = 0: the gradient of c * sum |x_recon - x| (c = S * l1_weight / n). */
int mebt_op_l1_seed(const float* x_recon, const float* x, float* out, int64_t n, float c, mebt_stream_t stream);
/* dz[m, :] = c * (z[m, :] - embeddings[ids[m], :]) + g_st[m, :]: the commitment term (c = S * 0.5 / numel(z)) plus the straight-through
 * gradient arriving at the quantised embeddings (codebook.py:64,91); g_st may be NULL.  All fp32 [M, d]. */
int mebt_op_vq_seed(const float* z, const float* embeddings, const int64_t* ids, const float* g_st, float* dz, int64_t M, int32_t d,
                    int32_t n_codes, float c, mebt_stream_t stream);

/* ---- frame ingest for pixel-space training (reference mebt/data.py FrameListDataset.getTensor) ------------------------------
 * Uint8 RGB frames [N, Hs, Ws, 3] (N = clips x T) -> crop [y0, y0 + S) x [x0, x0 + S) -> PIL Image.resize((R, R), BILINEAR) ->
 * float32(u) / 255 - 0.5 through `lut` [256] -> out [Bout, 3, T, R, R] fp32; clip i goes to slot slots[i] (NULL: slot i, a slot
 * outside [0, Bout) is skipped).  `tab` = xmin[R], n[R], k[R][K] int32: Pillow's fixed-point coefficients of the S -> R axis
 * (mebt_amd/frames.py:axis_coeffs), used for both axes; `rows` output rows per workgroup, whose source rows (at most `span`)
 * fit the LDS.  S == R: no resampling, `tab` may be NULL.  Integer arithmetic only: the result equals PIL's bit for bit. */
int mebt_op_frames_to_video(const uint8_t* frames, float* out, int32_t N, int32_t T, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0,
                            int32_t S, int32_t R, const int32_t* tab, int32_t K, int32_t rows, int32_t span, const float* lut,
                            const int32_t* slots, int32_t Bout, mebt_stream_t stream);
/* The same crop and resize with uint8 output for the real side of FVD / KVD (reference measure_fvd_with_numpy.py:63): the resampled
 * byte goes through the uint8 table `lut` [256] = ((float32(u) / 255 - 0.5 + 0.5) * 255).byte() (mebt_amd/frames.py:byte_table; not
 * the identity) -> out [Bout, T, R, R, 3] uint8, the clip layout of mebt_op_i3d_preprocess.  Every other argument as above.  No
 * floating point at all: the result equals the reference's bytes. */
int mebt_op_frames_to_clip_u8(const uint8_t* frames, uint8_t* out, int32_t N, int32_t T, int32_t Hs, int32_t Ws, int32_t y0, int32_t x0,
                              int32_t S, int32_t R, const int32_t* tab, int32_t K, int32_t rows, int32_t span, const uint8_t* lut,
                              const int32_t* slots, int32_t Bout, mebt_stream_t stream);
/* ---- packed frame datasets (mebt_amd/packed.py): clips gathered from a pack of prepared frames ------------------------------------
 * pack: uint8 [F, R, R, 3] in device memory, every frame after the crop and resize above; ids: int64 [B, T] on the device, row
 * numbers into the pack.  out [B, 3, T, R, R] fp32 = lut[pack[ids]] (`lut` [256] as for mebt_op_frames_to_video): given the same bytes,
 * what mebt_op_frames_to_video writes.  An id outside [0, F) writes nothing for that frame and reads nothing; all offsets into the
 * pack are 64-bit (a resident pack is tens of GB).  The pack pointer needs no alignment. */
int mebt_op_pack_to_video(const uint8_t* pack, int64_t F, const int64_t* ids, float* out, int32_t B, int32_t T, int32_t R,
                          const float* lut, mebt_stream_t stream);
/* The same gather through the uint8 table `lut` [256] -> out [B, T, R, R, 3] uint8, the clip layout of mebt_op_i3d_preprocess: given the
 * same bytes, what mebt_op_frames_to_clip_u8 writes. */
int mebt_op_pack_to_clip_u8(const uint8_t* pack, int64_t F, const int64_t* ids, uint8_t* out, int32_t B, int32_t T, int32_t R,
                            const uint8_t* lut, mebt_stream_t stream);
/* ---- decoded video -> uint8 clip: what the sampling scripts keep of a first-stage decode -------------------------------------------
 * in: fp32 [B, 3, Td, H, W], contiguous (VQGAN.decode); out: uint8 [B, T, H, W, 3], 1 <= T <= Td, the first T frames in the clip
 * layout of mebt_op_i3d_preprocess.  u = (uint8) trunc((min(max(x, -0.5f), 0.5f) + 0.5f) * 255.0f), float32 throughout with the add and
 * the multiply rounded separately: `torch.clamp(img, -0.5, 0.5) + 0.5` of the scripts, then numpy's float32 `* 255` and
 * `.astype(np.uint8)`, bit for bit.  +-inf follow the clamp (0 and 255); NaN writes 0.  All offsets are 64-bit; `out` needs no
 * alignment (rows of a larger store start at multiples of 3 T H W bytes). */
int mebt_op_video_to_clip_u8(const float* in, uint8_t* out, int32_t B, int32_t Td, int32_t T, int32_t H, int32_t W,
                             mebt_stream_t stream);
/* ---- reconstruction metrics of the first stage (reference VQGAN.validation_step, mebt/vqgan.py:190-196; codebook.py:64,93-94) ------
 * The sums behind val/recon_loss, val/commitment_loss, val/perplexity and the per-frame PSNR / SSIM of a reconstruction.  Results are
 * bitwise reproducible: every floating-point sum is taken per workgroup, written as an fp64 partial into the caller's `scratch` and
 * added by a second kernel in a fixed order (no float atomics); integer sums are exact in any order.  All offsets are 64-bit.  `scratch`
 * needs 8-byte alignment and at least the stated number of bytes (`scratch_bytes` is checked before anything is launched). */
#define MEBT_RECON_ABS_CHUNK 16384      /* elements of one clip per workgroup: 256 lanes x 64 terms */
#define MEBT_RECON_TILE_H 16            /* SSIM positions per workgroup: 16 rows x 32 columns */
#define MEBT_RECON_TILE_W 32
#define MEBT_RECON_CODE_ROWS 16         /* rows of z per workgroup */
/* out[b] = sum_i |x[b, i] - y[b, i]|, fp64; x, y fp32 [B, n] contiguous (a video and its decode, n = 3 T H W).  A lane adds at most 64
 * terms in fp32 before the partial is widened to fp64.  scratch: 8 * B * ceil(n / MEBT_RECON_ABS_CHUNK) bytes. */
int mebt_op_abs_diff_sum(const float* x, const float* y, double* out, int32_t B, int64_t n, void* scratch, int64_t scratch_bytes,
                         mebt_stream_t stream);
/* a, b: uint8 [N, H, W, 3], frames of two clips in the layout of mebt_op_i3d_preprocess.  sq_err[n] = sum (a - b)^2 over the frame
 * (int64, exact); ssim[n] (fp64) = the frame's mean SSIM (Wang et al. 2004): 11 x 11 Gaussian window, sigma 1.5 (g_i = exp(-(i - 5)^2 /
 * 4.5), normalised in fp64 on the host), valid positions only ((H - 10) x (W - 10), no padding), per channel on the byte values,
 * C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, mean over positions and the three channels.  The moments are taken in fp32 on u - 128
 * (variances are shift invariant) with the window applied as two separable passes through LDS.  H, W >= 11, else
 * MEBT_STATUS_ESHAPE.  scratch: 16 * N * ceil((H - 10) / MEBT_RECON_TILE_H) * ceil((W - 10) / MEBT_RECON_TILE_W) bytes. */
int mebt_op_clip_quality_u8(const uint8_t* a, const uint8_t* b, int64_t* sq_err, double* ssim, int32_t N, int32_t H, int32_t W,
                            void* scratch, int64_t scratch_bytes, mebt_stream_t stream);
/* ids int64 [M], z fp32 [M, d] (the activations the codebook search read), embeddings fp32 [n_codes, d].  hist int64 [n_codes] +=
 * the number of rows with each id (64-bit integer atomics: the caller zeroes it once and a data set accumulates over calls);
 * sq_sum[0] (fp64) = sum_m |z_m - e_ids[m]|^2 of this call.  A row whose id is outside [0, n_codes) counts for neither and its
 * embedding is never read.  scratch: 8 * ceil(M / MEBT_RECON_CODE_ROWS) bytes. */
int mebt_op_code_stats(const int64_t* ids, const float* z, const float* embeddings, int64_t* hist, double* sq_sum, int64_t M,
                       int32_t n_codes, int32_t d, void* scratch, int64_t scratch_bytes, mebt_stream_t stream);
/* ---- EMA codebook of first-stage training (reference mebt/modules/codebook.py:25-46,66-89; csrc/codebook/codebook_train.hip) ------
 * All three operators are bitwise reproducible: integer atomics only, every floating-point sum in a fixed order.  The update's
 * products, sums and quotients are separately rounded fp32 operations in the reference's order (no FMA contraction).  `scratch`
 * needs 16-byte alignment and the bytes the *_scratch_bytes function states (checked before anything is launched). */
int64_t mebt_codebook_sums_scratch_bytes(int64_t M, int32_t n_codes);
/* ids int64 [M], z fp32 [M, d] channels-last (what the codebook search read).  n_total[c] = the number of rows with id c (fp32
 * [n_codes]), encode_sum[c, :] = the sum of those rows of z (fp32 [n_codes, d]; zero for a code without rows): codebook.py:68-69
 * without the one-hot matrix.  An inverted index (histogram, exclusive scan, row list per code) is built with integer atomics in
 * `scratch`; one wave then adds a code's rows in ascending row order in fp32.  Ids outside [0, n_codes) are skipped.  Any d >= 1;
 * 16-byte loads where d % 4 == 0 and z / encode_sum are 16-byte aligned.  M < 2^31 - 256. */
int mebt_op_codebook_sums(const int64_t* ids, const float* z, float* n_total, float* encode_sum, int64_t M, int32_t n_codes, int32_t d,
                          void* scratch, int64_t scratch_bytes, mebt_stream_t stream);
int64_t mebt_codebook_ema_scratch_bytes(int32_t n_codes);
/* In place, all fp32: N = 0.99 N + 0.01 n_total; z_avg = 0.99 z_avg + 0.01 encode_sum; n = sum N (fixed-order tree);
 * weights = (N + 1e-7) / (n + n_codes * 1e-7) * n; embeddings = z_avg / weights; and, where k_rand [n_codes, d] is not NULL,
 * usage = N >= restart_thres, embeddings = embeddings * usage + k_rand * (1 - usage) (codebook.py:74-80,87-89).  restarted[0]
 * (int32, on the device) = the number of codes with usage 0, 0 without k_rand. */
int mebt_op_codebook_ema(float* N, float* z_avg, float* embeddings, const float* n_total, const float* encode_sum, const float* k_rand,
                         int32_t* restarted, int32_t n_codes, int32_t d, float restart_thres, void* scratch, int64_t scratch_bytes,
                         mebt_stream_t stream);
/* out[j, :] = z[src[j] mod M, :] + noise[j, :] * std, std = 0.01 / sqrt(d) rounded to fp32, the product rounded before the sum
 * (codebook.py:25-32,41,83: row src[j] of the tiled and permuted z); noise NULL: the plain rows (M >= n_codes, no tiling).  z fp32
 * [M, d], src int64 [n_codes], noise / out fp32 [n_codes, d]. */
int mebt_op_codebook_restart_rows(const float* z, const int64_t* src, const float* noise, float* out, int64_t M, int32_t n_codes, int32_t d,
                                  mebt_stream_t stream);
/* ---- Inception-I3D forward for FVD / KVD (reference mebt/fvd/pytorch_i3d.py, mebt/fvd/fvd.py) ---------------------------------
 * Activations are channels-last [B, T, H, W, C] of `dtype` (MEBT_DTYPE_F16: MFMA fast mode, MEBT_DTYPE_F32: parity mode).
 * Uint8 frames [N, H, W, 3] -> bilinear resize to [N, Ho, Wo, 3] (align_corners=False, source coordinate clamped at 0), then
 * 2 x / 255 - 1 (fvd.py:17-28). */
int mebt_op_i3d_preprocess(int32_t dtype, const uint8_t* in, void* out, int32_t N, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                           mebt_stream_t stream);
#define MEBT_I3D_MAX_SEGS 3
/* Output columns [n0, n1) of a convolution go to out[voxel * cstride + coff + (n - n0)] (a slice of a concatenated tensor). */
typedef struct mebt_i3d_seg {
    void* out;
    int32_t n0, n1, cstride, coff;
} mebt_i3d_seg;
/* Unit3D (pytorch_i3d.py:50-136) with eval-mode BatchNorm folded into w / bias: an implicit GEMM over K = k0 k1 k2 Cin (flat
 * (tap, ci) index, ci fastest).  in: contiguous channels-last [B, Ti, Hi, Wi, Cin]; w: [Npad][Kpad] of `dtype`, Npad = Cout rounded
 * up to 64, Kpad = K rounded up to 32, zero in the padding; bias fp32 [Cout] or NULL; relu 0 / 1.  Zero padding: output voxel o
 * reads input o * s - pad_front + tap, and the output size must equal (size + pad_front + pad_back - k) / s + 1 on every axis.
 * nseg (1..3) segments cover [0, Cout) in order; several segments run the 1x1 branches of an Inception module as one GEMM. */
typedef struct mebt_i3d_conv_desc {
    const void* in; const void* w; const float* bias;
    int32_t B, Ti, Hi, Wi, Cin, To, Ho, Wo, Cout;
    int32_t k[3], s[3], pad_front[3], pad_back[3];
    int32_t relu;
    int32_t nseg;
    mebt_i3d_seg seg[MEBT_I3D_MAX_SEGS];
} mebt_i3d_conv_desc;
int mebt_op_i3d_conv(int32_t dtype, const mebt_i3d_conv_desc* d, mebt_stream_t stream);
/* MaxPool3dSamePadding (pytorch_i3d.py:13-46): zero "same" padding, output [B, ceil(Ti/st), ceil(Hi/sh), ceil(Wi/sw), C]. */
int mebt_op_i3d_maxpool(int32_t dtype, const void* in, void* out, int32_t B, int32_t Ti, int32_t Hi, int32_t Wi, int32_t C, int32_t kt,
                        int32_t kh, int32_t kw, int32_t st, int32_t sh, int32_t sw, mebt_stream_t stream);
/* Head (pytorch_i3d.py:324-331), fp32: AvgPool3d([2, 7, 7], stride 1) of x [B, T, 7, 7, C] into pooled (scratch [B, T - 1, C]),
 * the logits 1x1x1 convolution (w fp32 [ncls][C], bias fp32 [ncls] or NULL), the mean over time into logits [B, ncls]. */
int mebt_op_i3d_head(int32_t dtype, const void* x, const float* w, const float* bias, float* pooled, float* logits, int32_t B, int32_t T,
                     int32_t H, int32_t W, int32_t C, int32_t ncls, mebt_stream_t stream);
/* ---- LPIPS: the VGG-16 perceptual distance of the first stage (reference mebt/modules/lpips.py; VQGAN.validation_step's
 * val/perceptual_loss, mebt/vqgan.py:104-107,190-196) ---------------------------------------------------------------------------------
 * Activations are channels-last [N, H, W, C] of `dtype` (MEBT_DTYPE_F16: MFMA fast mode, MEBT_DTYPE_F32: parity mode); accumulation is
 * fp32 in both.  All offsets are 64-bit; every entry checks its arguments before it launches and allocates nothing. */
/* ScalingLayer on chosen frames: video fp32 [B, 3, T, H, W] (the VQGAN boundary tensor), frames int32 [n_frames][2] = (b, t) on the
 * device -> out [n_frames, H, W, 3] = (x - shift[c]) / scale[c]: the subtraction, then the division, each rounded in fp32, then one
 * rounding to `dtype`.  shift, scale: three floats each in HOST memory.  A (b, t) outside the video reads nothing and writes zeros. */
int mebt_op_lpips_input(int32_t dtype, const float* video, const int32_t* frames, void* out, int32_t B, int32_t T, int32_t H, int32_t W,
                        int64_t n_frames, const float* shift, const float* scale, mebt_stream_t stream);
/* 3x3 convolution, stride 1, zero padding 1, bias (fp32 [Cout] or NULL), ReLU when relu != 0.  in [N, H, W, Cin], out [N, H, W, Cout];
 * w: [Cout rounded up to 64][Kpad] of `dtype`, K = 9 Cin as (tap, ci) with ci fastest, Kpad = K rounded up to 32, zeros in the padding:
 * the tensor mebt_op_i3d_conv takes for k = (1, 3, 3).  Cin == 3, or Cin a multiple of 32 up to 512; any N, H, W >= 1; in, w and out
 * 16-byte aligned.  A workgroup stages a patch of the map with its halo into LDS once per 32 input channels and serves the nine taps
 * from it.  The accumulation order of an output depends on nothing but Cin: an image gives the same bits alone and in any batch. */
int mebt_op_conv2d_3x3(int32_t dtype, const void* in, const void* w, const float* bias, void* out, int32_t N, int32_t H, int32_t W,
                       int32_t Cin, int32_t Cout, int32_t relu, mebt_stream_t stream);
/* nn.MaxPool2d(2, 2): in [N, H, W, C] -> out [N, H / 2, W / 2, C] (rounded down, no padding).  H or W < 2: MEBT_STATUS_ESHAPE. */
int mebt_op_maxpool_2x2(int32_t dtype, const void* in, void* out, int32_t N, int32_t H, int32_t W, int32_t C, mebt_stream_t stream);
#define MEBT_LPIPS_HEAD_ROWS 16         /* pixels per workgroup of the head */
/* One slice's term: feats [2 N, P, C] (N real images, then their N reconstructions; P = H W pixels), w fp32 [C] the slice's `lin`
 * weights.  v[n] = (1 / P) sum_p sum_c w[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2, |f| the L2 norm over channels
 * (normalize_tensor: the eps outside the root, so a zero vector contributes exactly 0); out[n] += v[n] (fp64: the caller zeroes it and
 * the five slices accumulate); layer_out (may be NULL): layer_out[n * layer_stride] = v[n].  Norms and the sum over channels are fp32
 * (at most ceil(C / 64) terms per lane), fp64 from there; one fp64 partial per workgroup, added in index order by a second kernel: no
 * float atomics, the same bits on every run.  scratch: 8-byte aligned, 8 * N * ceil(P / MEBT_LPIPS_HEAD_ROWS) bytes. */
int mebt_op_lpips_head(int32_t dtype, const void* feats, const float* w, double* out, double* layer_out, int64_t layer_stride, int64_t N,
                       int64_t P, int32_t C, void* scratch, int64_t scratch_bytes, mebt_stream_t stream);
/* ---- LPIPS backward: the perceptual term of first-stage training (csrc/lpips/lpips_bwd.hip; LPIPS.value_and_grad) -------
 * The network is frozen: data gradients only.  Same layouts and dtypes as the forward; arithmetic in fp32, stores in `dtype`.  No float
 * atomics and no reduction whose order depends on the launch: the same bits on every run, and an image's gradient does not depend on the
 * batch it ran in. */
/* Backward of one slice's term, for the reconstruction half only.  feats [2 N, P, C] and w as mebt_op_lpips_head reads them; add
 * [N, P, C] (may be NULL): the gradient arriving from the deeper slice through the next pool.  With d = |f| + 1e-10, k = -2 coef / P
 * (rounded to fp32 once on the host):  g_c = k w_c (f0_c / d0 - f1_c / d1),  df1_c = g_c / d1 - f1_c (sum_k g_k f1_k) / (|f1| d1^2)
 * (the second term 0 where |f1| = 0);  d_feats[n, p, c] = f1_c > 0 ? df1_c + add : 0 (the slice output is a ReLU output, so this is the
 * gradient at the last convolution's pre-activation).  One wave per pixel. */
int mebt_op_lpips_head_bwd(int32_t dtype, const void* feats, const float* w, const void* add, void* d_feats, int64_t N, int64_t P, int32_t C,
                           double coef, mebt_stream_t stream);
/* nn.MaxPool2d(2, 2) backward: in [N, H, W, C] (the pool's saved input, a ReLU output), dy [N, H / 2, W / 2, C] -> dx [N, H, W, C], every
 * element written (zeros in a trailing odd row or column).  dy goes to the first maximum of its window in row-major order (torch's
 * rule) where that maximum is positive; a window of zeros passes nothing on. */
int mebt_op_maxpool_2x2_bwd(int32_t dtype, const void* in, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                            mebt_stream_t stream);
/* Data gradient of mebt_op_conv2d_3x3: dy [N, H, W, Cin] (Cin = the forward's Cout, a multiple of 32 up to 512) -> dx [N, H, W, Cout]
 * (Cout = the forward's Cin, any value >= 1).  w_dgrad: [Cout rounded up to 64][Kpad] with the taps flipped and the channels swapped
 * (mebt_amd.lpips.arrange_weight_dgrad).  It is the forward's kernel without bias and ReLU; y_prev [N, H, W, Cout] (may be NULL) is the
 * forward output of the layer below and dx = y_prev > 0 ? acc : 0, the ReLU's backward fused.  All four pointers 16-byte aligned. */
int mebt_op_conv2d_3x3_dgrad(int32_t dtype, const void* dy, const void* w_dgrad, const void* y_prev, void* dx, int32_t N, int32_t H, int32_t W,
                             int32_t Cin, int32_t Cout, mebt_stream_t stream);
/* ScalingLayer backward: seed[b, c, t, y, x] += factor * (d_in[n, y, x, c] / scale[c]) for (b, t) = frames[n].  d_in [n_frames, H, W, 3]
 * of `dtype`; seed fp32 [B, 3, T, H, W] (what mebt_op_l1_seed writes); the division is rounded in fp32, then multiplied by `factor`, a
 * positive power of two (exact).  frames: int32 [n_frames][2] on the device; frames_host: the same pairs in HOST memory, which are
 * checked before the launch: a pair outside the video or a repeated pair is MEBT_STATUS_EINVAL (each seed element has one writer, so the
 * kernel is a plain read-modify-write).  scale: three floats in HOST memory. */
int mebt_op_lpips_input_bwd(int32_t dtype, const void* d_in, const int32_t* frames, const int32_t* frames_host, float* seed, int32_t B,
                            int32_t T, int32_t H, int32_t W, int64_t n_frames, const float* scale, float factor, mebt_stream_t stream);

/* ---- First-stage discriminators: BatchNorm statistics and loss values (csrc/disc/disc.hip; reference mebt/vqgan.py:27-37,416-520;
 * DESIGN.md §9i) ---------------------------------------------------------------------------------------------------------------------
 * Maps are channels-last [M, C] of `dtype` (MEBT_DTYPE_F16 or MEBT_DTYPE_F32); sums are fp64, offsets 64-bit, every entry checks its
 * arguments before it launches and allocates nothing.  No float atomics: the same input gives the same bits on every run. */
#define MEBT_DISC_BN_ROWS 128           /* rows per workgroup (= per slot) of the BatchNorm partials */
/* Per channel c and slot g the fp64 {sum, sum of squares} of rows [g R, (g + 1) R) of x [M, C], R = MEBT_DISC_BN_ROWS, at
 * slots[(c * 2 + q) * n_slots + g], n_slots = ceil(M / R); slots: 8-byte aligned, slots_bytes >= 16 * C * n_slots. */
int mebt_op_disc_bn_partials(int32_t dtype, const void* x, int64_t M, int32_t C, void* slots, int64_t slots_bytes, mebt_stream_t stream);
/* Adds each channel's n_slots slots in index order (fp64) -> stats fp32 [2][C] = mean, 1 / sqrt(max(var, 0) + 1e-5) with the biased
 * variance over `count` values per channel.  update != 0: running_mean / running_var (fp32 [C]) move by momentum 0.1 towards the mean
 * and the unbiased variance, *num_batches_tracked (int64 on the device, may be NULL) += 1: nn.BatchNorm's training-mode bookkeeping.
 * count < 2: MEBT_STATUS_ESHAPE ("expected more than 1 value per channel when training"). */
int mebt_op_disc_bn_finish(const void* slots, int64_t n_slots, int32_t C, int64_t count, float* stats, float* running_mean, float* running_var,
                           int64_t* num_batches_tracked, int32_t update, mebt_stream_t stream);
/* fp64 means in fixed order.  n_logits > 0: out[0..4] = mean of l, relu(1 - l), relu(1 + l), softplus(-l), softplus(l) over logits
 * [n_logits] of `dtype` (the halves of hinge_d_loss / vanilla_d_loss and the generator term).  n_feat > 0: out[5] = mean |a - b| of two
 * feature tensors [n_feat] of `dtype` (feature matching).  Entries not asked for are left alone.  scratch: 8-byte aligned,
 * mebt_disc_losses_scratch_bytes(n_logits, n_feat) bytes. */
int64_t mebt_disc_losses_scratch_bytes(int64_t n_logits, int64_t n_feat);
int mebt_op_disc_losses(int32_t dtype, const void* logits, int64_t n_logits, const void* feat_a, const void* feat_b, int64_t n_feat, double* out,
                        void* scratch, int64_t scratch_bytes, mebt_stream_t stream);

/* ---- First-stage discriminators: the forward (csrc/disc/disc_conv.hip, addressing in csrc/disc/disc_addr.h; reference
 * mebt/vqgan.py:416-520) ----------------------------------------------------------------------------------------------
 * Maps are channels-last [B, T, H, W, C] of `dtype` (T = 1 for the image network), 16-byte aligned.  A stage is the 4^d convolution
 * (kt 1 with Ti = 1, or kt 4), stride 1 or 2, zero padding 2 per side: To / Ho / Wo must equal n / 2 + 1 at stride 2 and n + 1 at
 * stride 1.  Cin is the channel count as stored: 4, or a multiple of the 16-byte vector (8 fp16, 4 fp32).  Weights are pre-arranged
 * [Npad][Kpad] of `dtype` (Npad = Cout rounded up to 64, Kpad = kt * 16 * Cin rounded up to 32, K order (tap, ci) with ci fastest, zeros
 * in the padding): w_bytes must be exactly that.  bias: fp32 [Cout].  Every entry checks its arguments in a fixed order before it
 * launches and allocates nothing; an output row's accumulation order does not depend on M, the batch or its tile. */
/* x fp32 [B, 3, T, H, W] -> out [B, To, H, W, 4] of `dtype`, fourth channel 0.  frame_idx NULL: To = T; else int64 [B] on the device,
 * each in [0, T) (the caller checks), To = 1: frame frame_idx[b] of clip b (vqgan.py:104-108). */
int mebt_op_disc_ingest(int32_t dtype, const float* x, const int64_t* frame_idx, void* out, int64_t out_bytes, int32_t B, int32_t T, int32_t H,
                        int32_t W, mebt_stream_t stream);
/* out [B, To, Ho, Wo, Cout] = conv(in) + bias, with LeakyReLU(0.2) when act != 0.  slots != NULL: also the BatchNorm partials of the
 * fp32 value (before the activation and before it is rounded to `dtype`), fp64 {sum, sum of squares} per channel and row tile in the
 * layout mebt_op_disc_bn_finish reads with n_slots = ceil(M / BM), BM = 128 (fp16) or 64 (fp32), M = B To Ho Wo; slots_bytes >=
 * 16 * Cout * n_slots. */
int mebt_op_disc_conv(int32_t dtype, const void* in, int64_t in_bytes, const void* w, int64_t w_bytes, const float* bias, void* out,
                      int64_t out_bytes, void* slots, int64_t slots_bytes, int32_t B, int32_t Ti, int32_t Hi, int32_t Wi, int32_t Cin, int32_t kt,
                      int32_t stride, int32_t To, int32_t Ho, int32_t Wo, int32_t Cout, int32_t act, mebt_stream_t stream);
/* In place on x [M, C] (C a multiple of 4): (x - mean) * rstd * gamma + beta, then LeakyReLU(0.2); stats fp32 [2][C] = mean, rstd as
 * mebt_op_disc_bn_finish writes them; gamma, beta fp32 [C]. */
int mebt_op_disc_bn_act(int32_t dtype, void* x, int64_t M, int32_t C, const float* stats, const float* gamma, const float* beta, mebt_stream_t stream);
/* The last stage (Cout 1, stride 1, no activation): out [B, To, Ho, Wo, 1]; w is the arranged [64][Kpad], of which row 0 is read. */
int mebt_op_disc_head(int32_t dtype, const void* in, int64_t in_bytes, const void* w, int64_t w_bytes, const float* bias, void* out,
                      int64_t out_bytes, int32_t B, int32_t Ti, int32_t Hi, int32_t Wi, int32_t Cin, int32_t kt, int32_t To, int32_t Ho, int32_t Wo,
                      mebt_stream_t stream);

/* ---- instrumentation ----------------------------------------------------------------------------- */
/* Per-kernel-family timing with HIP events on the launch stream (bench.py roofline): enable, run,
 * then read {launches, total ms, total algorithmic flops} of the GEMM family (family 0), or the
 * algorithmic operand + result bytes in place of the flops (family 1); family 2 / 3: the embedding gather forward /
 * its scatter-add backward with their algorithmic bytes. */
int mebt_profile_enable(int32_t on);
int mebt_profile_read(int32_t family, double* launches, double* total_ms, double* total_flops);
/* Every GEMM-family launch recorded while profiling was enabled, one text line each (`tag dims... ms gflop`; tag g = one product:
 * M N K a_kc b_kc epilogue c_f32; p = pair launch: M0 N0 K0 M1 N1 K1 b_kc; w = grouped weight gradients: items, output Ki-elements,
 * longest K).  Returns the bytes needed incl. the terminating 0 and writes the text when `cap` suffices (negative: HIP error). */
int64_t mebt_profile_dump(char* buf, int64_t cap);
/* Data parallel, while profiling is enabled: every wait of a forward for a deferred parameter gather
 * (mebt_model_set_forward_waits) is bracketed by an event pair.  Writes up to `cap` (first layer reading the bucket, ms the
 * compute stream stood still) pairs in launch order and returns how many were recorded (negative: HIP error). */
int32_t mebt_profile_read_waits(int32_t cap, int32_t* layer, double* ms);
/* Tests only: multiplies out[0..n) (fp32, n % 4 == 0) in place by the dropout keep-scales (0 or 1/(1-p))
 * of site `site` under `seed` — fill `out` with ones to read the mask the kernels use.  Site ids: 16*layer
 * + {0 attention probabilities, 1 proj output, 2 MLP output}; 0xFFFF0/1/2 = embedded sos/contexts/targets. */
int mebt_debug_dropout_mask(uint64_t seed, uint32_t site, float p, int64_t n, float* out, mebt_stream_t stream);
/* Diagnostics (bench.py): one wave on `stream` writes {s_memtime, s_memrealtime} at its start and again after `ref_ticks_100mhz`
 * ticks of the constant 100 MHz reference counter (<= 1 s) into out4[0..3]: (out4[2] - out4[0]) / (out4[3] - out4[1]) x 100 MHz is the
 * shader clock the GPU ran at in between, under whatever load the other streams put on it. */
int mebt_debug_clock_probe(unsigned long long* out4, uint64_t ref_ticks_100mhz, mebt_stream_t stream);
/* Benchmarking / tests only: 0 = keep every launch on the caller's stream (no side stream for gradient leaves). */
void mebt_debug_side_stream(mebt_model* m, int32_t on);
/* experiment: run that second stream's work on a caller-owned stream instead (NULL: back to the internal one) */
void mebt_debug_set_side_stream(mebt_model* m, mebt_stream_t stream);
/* Benchmarking / tests only: force the bf16 GEMM block tile: bm x bn one of 192x128, 128x128, 96x128, 128x64, 64x128, 96x64, 64x64 or
 * 256x256 (any other tile makes the launch fail with MEBT_STATUS_EINVAL); (0, 0) restores the tuned / heuristic choice. */
void mebt_debug_gemm_tile(int32_t bm, int32_t bn);
/* Benchmarking / tests only: force the bf16 GEMM variant (the low byte of a tune-table value): 0 register-staged, 2-5 LDS-DMA ring of
 * that depth (1 = 3), 8 + r the software-pipelined loop (r = 2-4), 16 + r two pipelines per workgroup (r = 2, 3), 32 + r / 64 + r split-K
 * in 2 / 4 fp32 slabs (r = 2, 3), with the 256 x 256 tile 9 the two staggered wave groups (anything else there: the 8-wave kernel).  A
 * variant the product cannot run falls back to the LDS-DMA ring of the tile.  100 + code: the same without the C store of plain
 * epilogues (199: the tuned / heuristic choice without it; experiments only).  -1 restores the tuned / heuristic choice. */
void mebt_debug_gemm_variant(int32_t dma);
/* Benchmarking only: a caller-owned device buffer (>= 496 MiB) the operator-level mebt_op_gemm may use as tuner /
 * split-K scratch (model-level entry points use their workspace); NULL removes it. */
void mebt_debug_gemm_scratch(void* buf, int64_t bytes);
/* Diagnostics only: with a device buffer of 4 x 8 bytes per workgroup installed, wave 0 of every workgroup of the plain bf16
 * GEMM kernels stamps s_memtime at entry / first k-tile landed / main loop done / epilogue stores retired (NULL: off). */
void mebt_debug_gemm_stamps(unsigned long long* buf);
/* Tests / benchmarking only: mebt_op_attention_fwd / _bwd apply attention dropout with probability p under `seed` (site 0; p = 0:
 * off, the default).  `dmask` (mebt_op_attention_fwd writes it, _bwd reads it; NULL: every kernel hashes) is a device buffer of
 * B * H * NQ * 32 * ceil(NK / 256) bytes for the shapes it is used with — the layout the model's training step uses. */
void mebt_debug_attn_dropout(uint64_t seed, float p, void* dmask);
/* Benchmarking / tests only: A/B of the bf16 attention launch forms.  bit 0: linear block order instead of the XCD-local one; bit 1:
 * the backward as two launches (dQ, then dK/dV) instead of one grid.  -1 restores the environment's choice (MEBT_ATTN_LEGACY, 0). */
void mebt_debug_attn_legacy(int32_t bits);
/* Tests only: the block order of the MFMA attention grids.  For a 1-D grid of T = X * H * B workgroups (X row blocks, H heads), workgroup
 * t writes t to pos_to_id[(b * H + h) * X + x] for the (x, h, b) it takes; xcd = 1 the XCD-local order, 0 the linear one. */
int mebt_debug_attn_block_order(int32_t T, int32_t X, int32_t H, int32_t xcd, int32_t* pos_to_id, mebt_stream_t stream);
/* Tests only: the form of the most recent bf16 MFMA attention forward.  Returns the number of such launches since the previous call;
 * out[4] (or NULL) = {waves per group (4 or 8), ring stages, split (0 = none, 1 = two groups in anti-phase: attn_fwd_pp, 2 = two groups
 * in phase), grid size}; all zero when there was none.  Process-wide and unsynchronised, like the other debug hooks. */
int32_t mebt_debug_attn_last_launch(int32_t out[4]);
/* Diagnostics (tools/wgrad_bench.py): every grouped weight-gradient launch uses this tile (128x128, 128x64, 64x128 or 64x64 with ring
 * 2-4; 256x128 with ring 2-3; a deeper ring is clamped) instead of the tuned / shipped choice, any other tile makes the launch fail with
 * MEBT_STATUS_EINVAL; tbm = 0 switches the override off. */
void mebt_debug_grouped_config(int32_t tbm, int32_t tbn, int32_t ring);
/* Tests only: while set, every launch that qualifies as a pair (mebt_op_gemm_pair) skips the tune table and runs the pair kernel of this
 * tile (192x128 with ring 2-3; 128x128, 96x128, 128x64, 64x128, 96x64 or 64x64 with ring 2-4; a deeper ring is clamped); any other tile
 * makes the launch fail with MEBT_STATUS_EINVAL and write nothing.  Products that do not qualify still go out as two ordinary
 * launches.  tbm = 0 switches the override off. */
void mebt_debug_pair_config(int32_t tbm, int32_t tbn, int32_t ring);
/* Tests only: the number of GEMM-family kernel launches (tuner candidates included) since the previous call; resets the count.  out[0..8)
 * describes the last of them: {family (0 single product, 1 pair, 2 grouped weight gradients, 3 split-K reduce; -1: none since the
 * previous call), code byte of the kernel that ran (see mebt_debug_gemm_variant; taken from its table entry, not from the request: the
 * 8-wave 256 x 256 kernel is 2, the fp32 kernels 0, the reduce kernels 32 / 64), block tile rows, block tile columns, threads per
 * workgroup, grid x, grid y, grid z}.  Process-wide and unsynchronised, like the other debug hooks. */
int32_t mebt_debug_gemm_last_launch(int32_t out[8]);
/* Benchmarking only: LDS-DMA ring depth (2 or 3) of the grouped weight-gradient GEMM. */
void mebt_debug_grouped_stages(int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* MEBT_HIP_H */

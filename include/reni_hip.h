/* reni_hip.h -- C ABI of libreni_hip.so: the MI355X (gfx950) RENI forward / training hot path.
 *
 * This is the drop-in boundary underneath the reference's nn.Module surface.  The reference
 * (JADGardner/RENI) has no FFI of its own; the seam it offers is the call
 *     model_output = self.model(Z, directions)            src/lightning/RENI_module.py:105 (training)
 *                                                          src/lightning/RENI_module.py:78  (inference)
 * into src/models/RENI.py (SO2/SO3/None invariant encoding :23-60, SineLayer :63-87, decoder
 * :132-178) plus the loss of src/utils/loss_functions.py:6-71 and the autograd backward of both.
 * Each entry point below names the reference code it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer on the current HIP device unless it says "host";
 *  - all tensors are fp32, row-major, contiguous unless a stride argument says otherwise;
 *  - `stream` is a hipStream_t passed as void* (0 = the null stream);
 *  - every function returns 0 on success or a negative RENI_E* code; the message of the last
 *    failure on the calling thread is available from reni_last_error();
 *  - the library allocates nothing per call: the caller owns params, gradients, I/O and the
 *    workspace (size from reni_workspace_bytes); the plan is immutable after creation.
 *
 * Flat parameter layout (`params`, `dparams`): the decoder's state_dict in the reference's own
 * order (src/models/RENI.py:132-178): net.0.linear.weight [H,F_in], net.0.linear.bias [H],
 * net.l.linear.weight [H,H], net.l.linear.bias [H] for l = 1..L, then the head weight [3,H] and
 * bias [3].  reni_param_count() gives the total.
 */
#ifndef RENI_HIP_H
#define RENI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RENI_OK 0
#define RENI_EINVAL (-1)       /* bad argument / unsupported shape */
#define RENI_EWORKSPACE (-2)   /* workspace too small */
#define RENI_EHIP (-3)         /* a HIP runtime call failed */
#define RENI_EUNSUPPORTED (-4) /* configuration not supported by the compiled kernels */

/* reni_desc.equivariance : which invariant encoding (src/models/RENI.py:118-126) */
#define RENI_EQ_NONE 0
#define RENI_EQ_SO2 1
#define RENI_EQ_SO3 2
/* reni_desc.output_activation (src/models/RENI.py:173-176) */
#define RENI_ACT_NONE 0
#define RENI_ACT_TANH 1
#define RENI_ACT_EXP 2
/* reni_desc.dtype : arithmetic of the dense layers */
#define RENI_F32 0  /* fp32 MFMA (v_mfma_f32_32x32x2_f32), precise sin/cos: bit-for-bit an fmaf chain */
#define RENI_BF16 1 /* bf16 MFMA (v_mfma_f32_32x32x16_bf16), fp32 accumulate, fp32 sin argument    */

/* reni_desc.conditioning : how the latent code conditions the SIREN (src/models/RENI.py:862, 877-933) */
#define RENI_COND_CONCAT 0 /* Cond-by-Concat: RENIAutoDecoder / RENIVariationalAutoDecoder      RENI.py:90-399  */
#define RENI_COND_FILM 1   /* FiLM: RENIAutoDecoderFiLM / RENIVariationalAutoDecoderFiLM         RENI.py:407-858 */

/* loss_kind for reni_forward_loss_backward */
#define RENI_LOSS_MSE 0  /* RENITrainLoss      = WeightedMSE                  loss_functions.py:6-13,39-45 */
#define RENI_LOSS_TEST 1 /* RENITestLoss       = MSE + alpha*|Z|^2 + beta*WeightedCosine  :25-32,60-71     */

/* flags */
#define RENI_NEED_DW 1u /* produce decoder gradients (dparams)                      */
#define RENI_NEED_DZ 2u /* produce latent gradients (dZ)                            */
/* The loss weight is zero over whole regions (RENI_module.py:92-94: sineweight * mask, the notebook's inpainting masks): the library
 * may leave out work that cannot change the result -- 128-pixel tiles whose weights are all zero, and the statistics pass of
 * RENITestLoss's cosine term for images whose pixel-0 weight is zero (loss_functions.py:25-32 multiplies the term by that weight).
 * The regions are found on the device from `weight` in every call; results are the dense ones (the skipped terms are exact zeros).
 * Honoured by the frozen-decoder calls of the concat models (no RENI_NEED_DW, no output image requested; every width, fp32 and bf16),
 * ignored elsewhere. */
#define RENI_WEIGHT_SPARSE 4u
/* As RENI_WEIGHT_SPARSE, and the pixels with weight are PACKED into each image's first tiles (a position -> pixel list built on the
 * device per call), so a tile is left out unless it holds such pixels: Mask-3 at 128 x 256 keeps 19 % of the pixels in 148 of 256
 * tiles -- packed, in 49.  The same terms are then summed in another order: results equal the dense ones to fp32 rounding, not bit
 * for bit (run-to-run they stay bit-identical). */
#define RENI_WEIGHT_COMPACT 8u
/* reni_latent_step_rows_cached only: the lists' build reported no image with a live cosine term (summary[2] == 0: pixel 0 of every
 * image is masked, as in every mask of the reference's data/Masks) -- the statistics pass and its per-image kernel, which would visit
 * nothing and write zero coefficients, are not launched.  Same results, two launches fewer. */
#define RENI_WEIGHT_COS_CONSTANT 16u

typedef struct reni_plan reni_plan;

typedef struct reni_desc {
  int32_t equivariance;      /* RENI_EQ_*                                   RENI.py:118-126 */
  int32_t ndims;             /* latent rows ND (Z is [ND,3])                RENI.py:94      */
  int32_t hidden_features;   /* H: 32, 64, 128 or 256                       RENI.py:96      */
  int32_t hidden_layers;     /* L: number of hidden SineLayers after the first (L+1 sine layers) RENI.py:143 */
  int32_t out_features;      /* must be 3                                    RENI.py:98      */
  int32_t last_layer_linear; /* 1: linear head, 0: sine head                RENI.py:153-171 */
  int32_t output_activation; /* RENI_ACT_*                                  RENI.py:173-176 */
  float first_omega_0;       /*                                             RENI.py:139     */
  float hidden_omega_0;      /*                                             RENI.py:149     */
  int32_t dtype;             /* RENI_F32 | RENI_BF16 */
  int32_t conditioning;      /* RENI_COND_*.  FiLM: hidden_layers = siren_hidden_layers - 1 (RENI.py:563-568),
                                omegas unused, last_layer_linear = 1                     RENI.py:537-570 */
  int32_t mapping_layers;    /* FiLM: hidden layers of the mapping network (0 = the reni_film_model_* entry points are
                                not used)                                                RENI.py:482-496 */
  int32_t mapping_features;  /* FiLM: width of those layers                             RENI.py:482-496 */
} reni_desc;

/* Message of the last error raised on this thread ("" if none). */
const char* reni_last_error(void);

/* Replaces the constructor of RENIAutoDecoder / RENIVariationalAutoDecoder as far as the decoder
 * is concerned (src/models/RENI.py:91-178): validates the hyper-parameters, selects kernels. */
int reni_plan_create(const reni_desc* desc, reni_plan** out_plan);
void reni_plan_destroy(reni_plan* plan);

/* Number of fp32 elements of the flat decoder parameter buffer; F_in via reni_in_features. */
int64_t reni_param_count(const reni_plan* plan);
int32_t reni_in_features(const reni_plan* plan);

/* Bytes of workspace the calls below need for (B images) x (P directions).  `flags` as passed
 * to the call (0 for reni_forward).  It scales with B x P only through per-tile buffers (a tile = 128 directions of one image):
 *   every backward path            8 KB of per-tile partials (not kept by the bf16 H = 128 training instance: image runs instead)
 *   bf16, H = 128, L <= 5          32 KB per tile: the g_1 stream (concat and FiLM; FiLM adds one partial slot per image RUN:
 *                                  <= 3 x #CUs x runs x 0.33 MB, independent of B x P)
 *   bf16, H = 128, L > 5           hidden_layers x 70 KB per tile: the operand-image stream (k_dw_stream)
 *   bf16, H = 256                  (2 L + 1) x 64 KB per tile: every tile's phase stash + the g_l fragment stream (k_dw_frag)
 *   fp32, H = 256, concat          (2 L + 1) x 128 KB per tile: the same in fp32 (k_dw_frag32)
 * e.g. 64 images x 32768 directions (16 384 tiles): 0.7 GB at 5 x 128, 11 GB at 5 x 256 bf16, 23 GB at 5 x 256 fp32.
 * (H = 256 training: a call whose stream would exceed 16 GB -- RENI_FRAG_WS_CAP_MB overrides -- runs in equal chunks of whole images,
 * one after the other, and the workspace is sized for one chunk: the fp32 example above is two passes of 32 images, 11.5 GB each.)
 * The H <= 128 stash ring and the per-workgroup gradient partials do not grow with B x P. */
size_t reni_workspace_bytes(const reni_plan* plan, int64_t B, int64_t P, uint32_t flags);

/* out[B,P,3] = model(Z, D) under no_grad -- replaces InvariantRepresentation + self.net(x)
 * (src/models/RENI.py:225-233) as called from RENI.forward (src/lightning/RENI_module.py:75-78).
 * Z [B,ND,3]; D [B,P,3] with `d_batch_stride` elements between images (0 = one shared grid
 * [P,3], which is what RENI_module.py:77 materialises with .repeat). */
int reni_forward(const reni_plan* plan, int64_t B, int64_t P, const float* Z, const float* D,
                 int64_t d_batch_stride, const float* params, float* out, void* ws,
                 size_t ws_bytes, void* stream);

/* Fused model(Z,D) -> loss -> backward: replaces RENI_module.py:105 + the criterion call
 * (:117 / :126-128) + loss.backward() for the decoder and latents.
 *   target  : element (b,p,c) at target[b*tgt_strides[0] + p*tgt_strides[1] + c*tgt_strides[2]]
 *             (accepts the channel-planar view of RENI_module.py:83-84 without a copy);
 *   weight  : sineweight (x mask), element (b,p,c) at weight[b*w_strides[0] + ...]; a stride of 0
 *             broadcasts (the reference .repeat's one [1,P,3] grid, RENI_module.py:90-94);
 *   loss_kind, alpha, beta : RENI_LOSS_*; alpha/beta only for RENI_LOSS_TEST;
 *   out     : optional [B,P,3] model output (NULL to skip the store);
 *   loss_terms[4] : (loss, mse, prior, cosine) summed over the batch as the reference does;
 *   dZ [B,ND,3]   : d loss / d Z   (written when flags & RENI_NEED_DZ);
 *   dparams       : flat decoder gradient, OVERWRITTEN (written when flags & RENI_NEED_DW). */
int reni_forward_loss_backward(const reni_plan* plan, int64_t B, int64_t P, const float* Z,
                               const float* D, int64_t d_batch_stride, const float* params,
                               const float* target, const int64_t tgt_strides[3],
                               const float* weight, const int64_t w_strides[3], int32_t loss_kind,
                               float alpha, float beta, uint32_t flags, float* out,
                               float* loss_terms, float* dZ, float* dparams, void* ws,
                               size_t ws_bytes, void* stream);

/* The same with the batch's latents given as ROWS OF A TABLE: image b uses Z_table[idx[b]] ([n_rows][ndims][3], idx on the
 * device) -- `Z = self.model.Z[idx, :, :]` of the training step (RENI_module.py:97-103) happens inside the prologue kernel
 * instead of as a separate gather.  dZ is [B][ndims][3] in batch order, as above.  An idx[b] outside [0, n_rows) cannot be
 * reported without a host synchronisation: it reads no memory outside the table, and image b's outputs, the loss terms and
 * every gradient of the call come out NaN (the reference's `Z[idx]` raises a device-side assert). */
int reni_forward_loss_backward_rows(const reni_plan* plan, int64_t B, int64_t P, const float* Z_table, int64_t n_rows, const int64_t* idx,
                                    const float* D, int64_t d_batch_stride, const float* params, const float* target,
                                    const int64_t target_strides[3], const float* weight, const int64_t weight_strides[3],
                                    int32_t loss_kind, float alpha, float beta, uint32_t flags, float* out,
                                    float* loss_terms, float* dZ, float* dparams, void* workspace, size_t workspace_bytes,
                                    void* stream);

/* One whole training step of the reference's FIT_DECODER loop in one call (RENI_module.py:80-146 training_step, :178-192 the
 * optimiser over decoder + latent table; run.py's `trainer.fit` iteration): reni_forward_loss_backward_rows with
 * RENI_NEED_DW | RENI_NEED_DZ, THEN reni_adam_step2 -- same arguments, same results, bit for bit -- in fewer launches:
 *   - the optimiser step is one launch that also sums layer 1's weight-gradient partials (on the persistent bf16 path their
 *     reduction is otherwise a launch of its own behind k_reni_dw1);
 *   - the NEXT batch's prologue (`idx_next`: its latent rows gathered, A_b, layer-0 operands, the packed weight images of the
 *     UPDATED decoder) is run at the end of this call, so the next call starts with its main kernel.
 * `stage_state` (in / out, zero before the first call) says whether -- and into which of two copies -- the previous call staged this
 * call's prologue.  The caller resets it to zero whenever it changes B, P, `params` or `Z_table` between two calls, and passes as
 * idx what it announced as `idx_next`: the library checks the indices on the device -- on every path, persistent and generic kernels alike --
 * and SKIPS a step whose batch is not the staged one, loudly: loss terms and the latent gradient come out NaN, and parameters,
 * latent table and all four Adam moments stay exactly as they were (the optimiser launch reads the check's flag).  The staged copies
 * live in `workspace`: ANY other library call that is given the same workspace between two calls of this function (a validation
 * forward, a fused loss, another B or P) overwrites them -- reset `stage_state` to zero after such a call (reni_amd/ops.py counts
 * its workspace hand-outs and does).  idx_next = NULL: nothing is staged (the next call runs its own prologue).  Z_table and params are
 * updated in place; dZ [B,ND,3] and dparams receive the step's gradients as reni_forward_loss_backward_rows returns them.  One
 * process; the data-parallel step is reni_train_step_rows_dp below. */
int reni_train_step_rows(const reni_plan* plan, int64_t B, int64_t P, float* Z_table, int64_t n_rows, const int64_t* idx,
                         const int64_t* idx_next, const float* D, int64_t d_batch_stride, float* params, const float* target,
                         const int64_t target_strides[3], const float* weight, const int64_t weight_strides[3], int32_t loss_kind,
                         float alpha, float beta, float* m_dec, float* v_dec, float* m_lat, float* v_lat, float lr, float b1,
                         float b2, float eps, int64_t step, float grad_scale, uint32_t* stage_state, float* loss_terms, float* dZ,
                         float* dparams, void* workspace, size_t workspace_bytes, void* stream);

/* The same step for one rank of a DATA-PARALLEL job (BASELINE config 3; the reference: PyTorch-Lightning's DDP strategy, run.py:97-110,
 * whose all-reduce averages the shared decoder's gradients over the ranks between backward and optimizer.step): everything
 * reni_train_step_rows does, with the exchange INSIDE the call -- fwd + loss + bwd, the partial reductions, an in-place RCCL
 * all-reduce(sum) of the flat decoder gradient on `comm` (reni_rccl_comm_create; the caller's stream), the one optimiser launch with
 * `grad_scale` (pass 1 / world_size: the mean), the next batch's prologue.  Same launches as the one-process step plus layer 1's
 * partial reduction (its sum must be in the gradient buffer before the collective) plus the collective.  The latent table needs no
 * exchange: every image's row has exactly one owner (reni_amd/dist.py).  dparams returns the SUM over the ranks.
 * overlap != 0: the gradient of layers >= 2 + head (final before the ring kernel runs) is all-reduced on the library's own
 * communication stream beside the rest of the backward pass, the remainder (first layer, layer 1) behind it on the caller's stream --
 * two collectives on `comm`, issued in the same order on every rank; element for element the same sums.
 * With a one-rank communicator the results are bit-equal to reni_train_step_rows (tests/test_gpu_dist.py).
 * The skip decision of a staged step (see reni_train_step_rows) is all-reduced with MAX over `comm` in front of the gradient -- one
 * more 4-byte collective per call, issued on every rank whether or not its own step was staged: a batch that is not the staged one on
 * ANY rank skips the step on EVERY rank (the replicas stay replicas); on a skipped step the layer-1 slice of dparams, which this
 * call's optimiser launch would have written, is NaN like the rest of the gradient. */
int reni_train_step_rows_dp(const reni_plan* plan, int64_t B, int64_t P, float* Z_table, int64_t n_rows, const int64_t* idx,
                            const int64_t* idx_next, const float* D, int64_t d_batch_stride, float* params, const float* target,
                            const int64_t target_strides[3], const float* weight, const int64_t weight_strides[3],
                            int32_t loss_kind, float alpha, float beta, float* m_dec, float* v_dec, float* m_lat, float* v_lat,
                            float lr, float b1, float b2, float eps, int64_t step, float grad_scale, void* comm, int32_t overlap,
                            uint32_t* stage_state, float* loss_terms, float* dZ, float* dparams, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Backward for an arbitrary upstream gradient dout[B,P,3] (generic autograd use of
 * model(Z,D)); the forward is recomputed inside the same fused kernel. */
int reni_backward(const reni_plan* plan, int64_t B, int64_t P, const float* Z, const float* D,
                  int64_t d_batch_stride, const float* params, const float* dout, uint32_t flags,
                  float* dZ, float* dparams, void* ws, size_t ws_bytes, void* stream);

/* ---- FiLM conditioning (src/models/RENI.py:407-858) ------------------------------------------------
 * The per-SAMPLE work of RENI*FiLM.forward_with_frequencies_phase_shifts (RENI.py:665-676, FiLMLayer
 * :508-519) runs in the fused kernels; the per-IMAGE glue stays with the caller (reni_amd/film.py):
 *   - the mapping network (RENI.py:470-505) is evaluated once per image -- the reference evaluates it per
 *     pixel on repeated rows (RENI.py:413-447), same values -- giving freq = 15 f + 30 and phase (RENI.py:666);
 *   - the first FiLMLayer acts on Siren_Input = [|d_xz|, d_y, D_xz Z_xz^T] (SO2, RENI.py:441) or D Z^T (SO3,
 *     RENI.py:410), which is linear in (dx, dy, dz, r): theta_0 = A_b (dx, dy, dz, r, 1) with the per-image
 *     A [B,H,8] (columns dx, dy, dz, r, 1, 3 unused) = freq_0 . (W_0 x + b_0) + phase_0 folded by the caller.
 * Flat `params`: net.0.layer.weight [H,F0], net.0.layer.bias [H] (unused by the kernels), net.l.layer.weight
 * [H,H], .bias [H] for l = 1..L, final_layer.weight [3,H], .bias [3];  F0 = reni_in_features().
 * film [B,L,2,H]: film[b][l-1][0] = freq, [1] = phase of hidden FiLM layer l of image b.
 * Gradients: dA [B,H,8] (d loss / d A), dfilm [B,L,2,H], dparams (flat; the net.0 slot is zero-filled --
 * its gradient follows from dA in the caller's glue).  loss_terms = (mse + cosine, mse, 0, cosine): the
 * latent prior of RENITestLoss (alpha |Z|^2) is the caller's. */
int reni_film_forward(const reni_plan* plan, int64_t B, int64_t P, const float* D, int64_t d_batch_stride,
                      const float* A, const float* film, const float* params, float* out, void* ws,
                      size_t ws_bytes, void* stream);
int reni_film_forward_loss_backward(const reni_plan* plan, int64_t B, int64_t P, const float* D,
                                    int64_t d_batch_stride, const float* A, const float* film,
                                    const float* params, const float* target, const int64_t tgt_strides[3],
                                    const float* weight, const int64_t w_strides[3], int32_t loss_kind,
                                    float beta, uint32_t flags, float* out, float* loss_terms, float* dA,
                                    float* dfilm, float* dparams, void* ws, size_t ws_bytes, void* stream);
int reni_film_backward(const reni_plan* plan, int64_t B, int64_t P, const float* D, int64_t d_batch_stride,
                       const float* A, const float* film, const float* params, const float* dout,
                       uint32_t flags, float* dA, float* dfilm, float* dparams, void* ws, size_t ws_bytes,
                       void* stream);

/* FiLM, whole model: the per-image glue of the three calls above runs in HIP too (k_film_minput / _linear / _fold,
 * k_film_dout / _linear_t / _grads), so these take the latent codes and the mapping network's parameters and return
 * their gradients -- the drop-in for RENI*FiLM.forward (RENI.py:628-676) + criterion + loss.backward().
 *   map_params / dmap_params : mapping_network.network.{0,2,...}.{weight [N_i,K_i], bias [N_i]} flat, in state-dict
 *                              order (RENI.py:482-496); reni_film_map_param_count() elements;
 *   dparams                  : flat net.* / final_layer.* gradient INCLUDING the first layer's slot;
 *   loss_terms               : (loss, mse, prior, cosine) with prior = alpha |Z|^2 (RENI_LOSS_TEST). */
int64_t reni_film_map_param_count(const reni_plan* plan);
int reni_film_model_forward(const reni_plan* plan, int64_t B, int64_t P, const float* Z, const float* D,
                            int64_t d_batch_stride, const float* params, const float* map_params, float* out,
                            void* ws, size_t ws_bytes, void* stream);
int reni_film_model_forward_loss_backward(const reni_plan* plan, int64_t B, int64_t P, const float* Z, const float* D,
                                          int64_t d_batch_stride, const float* params, const float* map_params,
                                          const float* target, const int64_t tgt_strides[3], const float* weight,
                                          const int64_t w_strides[3], int32_t loss_kind, float alpha, float beta,
                                          uint32_t flags, float* out, float* loss_terms, float* dZ, float* dparams,
                                          float* dmap_params, void* ws, size_t ws_bytes, void* stream);
int reni_film_model_backward(const reni_plan* plan, int64_t B, int64_t P, const float* Z, const float* D,
                             int64_t d_batch_stride, const float* params, const float* map_params, const float* dout,
                             uint32_t flags, float* dZ, float* dparams, float* dmap_params, void* ws, size_t ws_bytes,
                             void* stream);

/* torch.optim.Adam(lr, betas=(b1,b2), eps) step on a flat buffer (RENI_module.py:192: the
 * reference always uses the default betas (0.9, 0.999), eps 1e-8).  `step` is the 1-based step
 * count; g is multiplied by grad_scale first (1/world_size after a sum all-reduce). */
int reni_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1,
                   float b2, float eps, int64_t step, float grad_scale, void* stream);

/* One iteration of the reference's FIT_LATENT loop -- the test-time optimisation of examples.ipynb cell 4: training_step with a fixed
 * decoder (RENI_module.py:92-103, 126-128), loss.backward(), Adam on the latent table (:178-192) -- in one call:
 * reni_forward_loss_backward_rows with flags = RENI_NEED_DZ | `flags`, THEN reni_adam_rows_step(Z_table, dZ, idx, ...) with
 * grad_scale 1 -- same arguments, same results.  `flags`: 0, RENI_WEIGHT_SPARSE or RENI_WEIGHT_COMPACT (a masked weight).
 * Z_table, m_lat, v_lat are updated in place; dZ [B,ND,3] receives the step's gradient; concat plans, one process. */
int reni_latent_step_rows(const reni_plan* plan, int64_t B, int64_t P, float* Z_table, int64_t n_rows, const int64_t* idx, const float* D,
                          int64_t d_batch_stride, const float* params, const float* target, const int64_t target_strides[3],
                          const float* weight, const int64_t weight_strides[3], int32_t loss_kind, float alpha, float beta,
                          uint32_t flags, float* m_lat, float* v_lat, float lr, float b1, float b2, float eps, int64_t step,
                          float* loss_terms, float* dZ, void* workspace, size_t workspace_bytes, void* stream);

/* The lists RENI_WEIGHT_SPARSE / RENI_WEIGHT_COMPACT work from -- which tiles carry weight, which images' cosine term is live, and
 * (COMPACT) the position -> pixel map -- depend on the loss weight alone, and the inpainting mask of a FIT_LATENT run is constant
 * over its 2 400 epochs (/root/reference/configs/experiment.yaml:47-48; RENI_module.py:92-94 multiplies the same mask into the sine
 * weight every step).  reni_latent_step_rows rebuilds them from the weight in every call (two or three dependent launches and an
 * 8 MB read in front of a 0.2 ms step); here the caller builds them ONCE into a buffer of its own and hands them to every step:
 *   reni_weight_lists_bytes(B, P)            size of the buffer (256-byte aligned device memory);
 *   reni_weight_lists_build(...)             fills it for this weight, these strides and `flags` (SPARSE or COMPACT), on `stream`;
 *                                            optionally reports what the lists hold (one synchronisation);
 *   reni_latent_step_rows_cached(..., lists) reni_latent_step_rows with the list-building launches left out: the same kernels on the
 *                                            same lists, results BIT-EQUAL to the rebuilt-every-call entry point.
 * The caller rebuilds the lists whenever the weight, B or P changes; `flags` of the step = `flags` of the build.
 * The library remembers, on the host, which buffers reni_weight_lists_build filled for which (B, P, mode) -- the last 64 builds --
 * and reni_latent_step_rows_cached returns RENI_EINVAL for a buffer it has no record of or that was built for another shape or mode
 * (the lists' layout depends on B and P: read at another shape they would be left).  What the record cannot see is a weight that
 * changed under unchanged lists. */
size_t reni_weight_lists_bytes(int64_t B, int64_t P);
/* summary_host (optional, 3 ints): after ONE stream synchronisation -- tiles the main pass will visit, tiles of the statistics pass,
 * images whose cosine term is live (0: the steps may carry RENI_WEIGHT_COS_CONSTANT). */
int reni_weight_lists_build(int64_t B, int64_t P, const float* weight, const int64_t weight_strides[3], uint32_t flags, void* lists,
                            size_t lists_bytes, int32_t* summary_host, void* stream);
int reni_latent_step_rows_cached(const reni_plan* plan, int64_t B, int64_t P, float* Z_table, int64_t n_rows, const int64_t* idx,
                                 const float* D, int64_t d_batch_stride, const float* params, const float* target,
                                 const int64_t target_strides[3], const float* weight, const int64_t weight_strides[3],
                                 int32_t loss_kind, float alpha, float beta, uint32_t flags, const void* weight_lists, float* m_lat,
                                 float* v_lat, float lr, float b1, float b2, float eps, int64_t step, float* loss_terms, float* dZ,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* The same Adam step over a table p [n_rows][row_len] whose gradient is given for the B rows idx[0..B) only
 * (g_rows [B][row_len], idx int64 on the device; repeated indices accumulate).  All other rows have gradient zero and
 * still move by their momentum: the dense torch.optim.Adam over the whole latent table that the reference runs
 * (RENI_module.py:178-192 puts model.Z / model.mu, all N rows, into the optimiser; a batch touches B of them). */
int reni_adam_rows_step(float* p, const float* g_rows, const int64_t* idx, int64_t B, int64_t row_len, float* m, float* v,
                        int64_t n_rows, float lr, float b1, float b2, float eps, int64_t step, float grad_scale,
                        void* stream);

/* One launch for both updates of a training step: reni_adam_step on the flat decoder buffer (p, g, m, v, n) and
 * reni_adam_rows_step on the latent table (table, g_rows, idx, B, row_len, tm, tv, n_rows) with the same
 * hyper-parameters -- the reference has ONE torch.optim.Adam over the decoder and the latent table (RENI_module.py:178-192). */
int reni_adam_step2(float* p, const float* g, float* m, float* v, int64_t n, float* table, const float* g_rows,
                    const int64_t* idx, int64_t B, int64_t row_len, float* tm, float* tv, int64_t n_rows, float lr, float b1,
                    float b2, float eps, int64_t step, float grad_scale, void* stream);

/* Self-test of the MFMA fragment layouts the kernels rely on; out (host pointer) receives the
 * number of mismatching elements per probe (0 = layout as assumed). */
int reni_selftest_layouts(int32_t* out_host_mismatch, int32_t n_probes);

/* Optional timing of the fused main kernel (the dominant kernel of the path) with HIP events recorded
 * on the caller's stream around each launch.  reni_profile_read synchronises the recorded events and
 * returns their summed duration and count since the last reset.  Used by bench.py for `roofline`. */
int reni_profile_enable(int32_t on);
int reni_profile_read(double* total_ms, int64_t* launches, int32_t reset);
/* The same, restricted to one kind of launch: 0 fused forward+loss+backward (what reni_profile_read returns),
 * 1 the statistics pass of RENITestLoss's cosine term, 2 plain inference (reni_forward), 3 the kernel that finishes the
 * backward pass from the g_1 stream behind the persistent training kernel (k_reni_l0_ring / k_reni_dw1_ring / k_reni_dw1),
 * 4 the weight-gradient consumers of the fragment / operand streams (k_dw_frag, k_dw_frag32, k_dw_stream, k_wide_head_dw),
 * 5 the data-parallel exchange inside reni_train_step_rows_dp (the skip flag's and the gradient's all-reduce, on the caller's stream),
 * -1 all of them. */
int reni_profile_read_kind(int32_t kind, double* total_ms, int64_t* launches, int32_t reset);
/* Shortest and longest launch of one kind among those recorded since the last reset (bench.py prints them beside the average:
 * boxes of the pool differ by several per cent, a cross-round delta is read against that spread).  Does not reset. */
int reni_profile_minmax(int32_t kind, double* min_ms, double* max_ms);

/* Diagnostic probe of the LDS transpose-read instruction (ds_read_b64_tr_b16): LDS holds u16 element i = i;
 * lane l reads at byte address 8*l (mode 0) or lane_addr_host[l] (mode 1); out_host[4*l + e] = element e. */
int reni_probe_tr(const int32_t* lane_addr_host, int32_t mode, uint16_t* out_host);

/* ---- environment-map Blinn-Phong shading of a G-buffer (FIT_INVERSE task) ------------------------------------
 * Replaces the arithmetic of blinn_phong_shading_env_map (src/utils/pytorch3d_envmap_shader.py:46-116) behind the
 * two interpolate_face_attributes calls (:68-73): the caller hands over the per-pixel interpolated vertex normals
 * and positions (the rasteriser is pytorch3d's, outside this library).
 *   normals, positions : [NP][3] device, NP = render pixels; NOT normalised (the library applies F.normalize(eps=1e-6)
 *                        as :82,:93 do); rows of zeros where no face covers the pixel (pix_to_face < 0)
 *   cam_*              : cameras.get_camera_center() (:78)
 *   light_dirs         : [J][3] unit directions of the environment-map texels (EnvironmentMap.directions, :75) of image
 *                        b at light_dirs + b * dirs_batch_stride (floats; 0 = one grid shared by all images, which is
 *                        what the reference's directions.repeat(B,1,1) amounts to, RENI_module.py:376)
 *   light_colors       : [B][J][3] EnvironmentMap.environment_map = map * sineweight (:41,:77)
 *   shininess, kd, ks  : materials.shininess (:79, 500 in build_renderer :186), kd, ks = 1 - kd (:199)
 *   colors             : [B][NP][3] = kd * diffuse + (s+2)/(4(2-exp(-s/2))) * ks * specular   (:112-115)
 * reni_envmap_shade_backward returns d loss / d light_colors [B][J][3] for an upstream d loss / d colors [B][NP][3]
 * (the only tensor of the shader that carries a gradient in the reference: the mesh and the grid are constants).
 * ws: reni_envmap_shade_workspace_bytes(B, NP, J) bytes, 256-byte aligned, for the partial sums. */
size_t reni_envmap_shade_workspace_bytes(int64_t B, int64_t NP, int64_t J);
int reni_envmap_shade(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                      float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                      const float* light_colors, float shininess, float kd, float ks, float* colors, void* ws,
                      size_t ws_bytes, void* stream);
int reni_envmap_shade_backward(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                               float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                               const float* dcolors, float shininess, float kd, float ks, float* dlight_colors, void* ws,
                               size_t ws_bytes, void* stream);

/* ---- mesh pipeline in front of the shader: vertex normals, camera, rasteriser, interpolation (FIT_INVERSE task) -----
 * Replaces what build_renderer (src/utils/pytorch3d_envmap_shader.py:177-217) takes from pytorch3d after load_obj, for one
 * mesh and one face per pixel: Meshes.verts_normals_packed, FoVPerspectiveCameras (fov 60, znear 1, zfar 100, aspect 1),
 * MeshRasterizer(blur_radius = 0, faces_per_pixel = 1, perspective_correct = False, no culling) and the shader's two
 * interpolate_face_attributes calls (:68-73).  fp32, deterministic (no float atomics: two calls give identical bits).
 *   verts        : [V][3] world positions; faces: [F][3] int64 vertex indices (a face with an index outside [0, V) is skipped)
 * reni_mesh_vertex_normals: normals[v] = s / max(|s|, 1e-6), s = sum of cross(v1 - v0, v2 - v0) over the faces of v, summed
 *   in ascending face order.  vf_offsets [V+1] / vf_corners: the faces of vertex v as corner indices 3 f + k with
 *   faces[f][k] == v, ascending, at vf_corners[vf_offsets[v] .. vf_offsets[v+1]) (entries that do not fit are ignored).
 * reni_rasterize_mesh: R [9] row-major and T [3] (host memory) give p_view = p_world R + T (row vectors, look_at_view_transform's
 *   convention); NDC x, y = view x, y / (view z * tan_half_fov), depth = view z, no clipping.  H == W = S; pixel (row, col) sits at
 *   NDC (-1 + (2 (S-1-col) + 1) / S, -1 + (2 (S-1-row) + 1) / S).  Per pixel p = row * S + col, nearest covering face (exact depth
 *   tie: the lower face index):
 *     pix_to_face [S*S] int64 (-1 background), zbuf [S*S], bary [S*S][3] (NDC, not perspective-corrected), dists [S*S] (minus the
 *     squared NDC distance to the face's edges), pixel_normals / pixel_positions [S*S][3] = the winner's barycentric interpolation
 *     of vert_normals / verts (not normalised).  Background: -1 in pix_to_face, zbuf, bary and dists, 0 in the two G-buffers.
 *   ws: reni_raster_workspace_bytes(V, F, H, W) bytes, 256-byte aligned (the per-face records). */
size_t reni_raster_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W);
int reni_mesh_vertex_normals(int64_t V, int64_t F, const float* verts, const int64_t* faces, const int64_t* vf_offsets,
                             const int64_t* vf_corners, float* normals, void* stream);
int reni_rasterize_mesh(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* vert_normals,
                        const float* R, const float* T, float tan_half_fov, int64_t H, int64_t W, int64_t* pix_to_face,
                        float* zbuf, float* bary, float* dists, float* pixel_normals, float* pixel_positions, void* ws,
                        size_t ws_bytes, void* stream);

/* ---- backward of the mesh G-buffer: pixel normals / positions -> vertex positions (reni_tu_raster_bwd.hip) ------------
 * The "interpolate" half of a differentiable rasteriser: pix_to_face is held fixed (no silhouette or occlusion gradient),
 * the camera is a constant.  Definitions, restating reni_tu_raster.hip (E = the edge function
 * E(p, a, b) = (p_x - a_x)(b_y - a_y) - (p_y - a_y)(b_x - a_x)):
 *   projection      q_i = p_i R + T,  t = tan_half_fov,  x_i = q_ix / (q_iz t),  y_i = q_iy / (q_iz t)
 *   barycentrics    pixel p with centre (px, py) and face f = (i0, i1, i2):  A = E((x2,y2), (x0,y0), (x1,y1)) + 1e-8,
 *                   w0 = E(p, 1, 2) / A,  w1 = E(p, 2, 0) / A,  w2 = E(p, 0, 1) / A
 *   interpolation   N_p = sum_k w_k n_ik,  X_p = sum_k w_k p_ik   (no perspective correction)
 *   vertex normals  n_v = u_v / max(|u_v|, 1e-6),  u_v = sum over the corners (f, k) naming v of
 *                   (p_f1 - p_f0) x (p_f2 - p_f0), over faces whose three indices are in range (k_vertex_normals' rule)
 * Computed, for gN, gX [S*S][3]:   g_verts = d/dp  sum_p (gN_p . N_p + gX_p . X_p)        [V][3]
 * differentiated as written: 1e-8 is a constant; in the max branch (|u| <= 1e-6) dn/du = I 1e6.  Four paths reach p: the
 * direct weights w_k of X_p; n_ik, through the normalisation and the cross products, to all vertices of all incident faces;
 * w_k -> (x, y) of the three corners, A included; (x, y) -> q -> p with d/dp_i = sum_j R[i][j] d/dq_j.  Background pixels
 * (pix_to_face -1) add nothing; a face the forward skips (an index outside [0, V), max view z < 0, |area| <= 1e-8) adds
 * nothing through the pixel paths but still through the vertex-normal path when its indices are in range; a vertex no face
 * names gets exactly 0.  fp32, no float atomics: every sum has one fixed order and two calls give identical bits.
 * Malformed input (an index outside [0, V), a list entry outside [0, 3F) or [0, S*S), a pix_to_face outside [-1, F)) adds
 * nothing and is never turned into an address.
 * reni_mesh_vertex_normals_backward: the vertex-normal chain alone, grad_verts [V][3] = d/dp sum_v grad_normals[v] . n_v;
 *   vf_offsets / vf_corners as for reni_mesh_vertex_normals.
 * reni_gbuffer_backward: R, T (host memory), tan_half_fov, H == W = S and pix_to_face [S*S] as reni_rasterize_mesh took and
 *   gave them; vert_normals [V][3] the normals it interpolated.  face_pixel_list [S*S]: the pixel indices in ascending
 *   order of their face (a stable sort of pix_to_face), face_pixel_offsets [F+1]: face f's pixels are
 *   face_pixel_list[face_pixel_offsets[f] .. face_pixel_offsets[f+1]).  The weights w_k are recomputed from the projected
 *   corners exactly as the forward computes them; `bary` is not read.  grad_pixel_normals / grad_pixel_positions [S*S][3]:
 *   either may be NULL (taken as 0), not both.  grad_verts [V][3] is overwritten.
 *   ws: reni_gbuffer_backward_workspace_bytes(V, F, H, W) bytes, 256-byte aligned (the per-face records, g u_v). */
int reni_mesh_vertex_normals_backward(int64_t V, int64_t F, const float* verts, const int64_t* faces, const int64_t* vf_offsets,
                                      const int64_t* vf_corners, const float* grad_normals, float* grad_verts, void* stream);
size_t reni_gbuffer_backward_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W);
int reni_gbuffer_backward(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* vert_normals,
                          const float* R, const float* T, float tan_half_fov, int64_t H, int64_t W, const int64_t* pix_to_face,
                          const int64_t* face_pixel_offsets, const int64_t* face_pixel_list, const int64_t* vf_offsets,
                          const int64_t* vf_corners, const float* grad_pixel_normals, const float* grad_pixel_positions,
                          float* grad_verts, void* ws, size_t ws_bytes, void* stream);

/* ---- soft silhouette: a differentiable coverage mask of the mesh and its vertex gradient (reni_tu_silhouette.hip) -------
 * What the G-buffer backward above leaves out: the gradient that moves the outline.  The classic soft coverage of SoftRas and
 * pytorch3d's SoftSilhouetteShader, restated from their documented behaviour.  Camera, projection, H == W = S, pixel
 * p = row * S + col and its NDC centre (px, py): exactly reni_rasterize_mesh's.  sigma > 0 and blur_radius r >= 0, both finite;
 * r is in squared NDC units.
 *   taking part     face f takes part iff reni_rasterize_mesh does not skip it for its indices or its area (every index in
 *                   [0, V), |area| > 1e-8), all three view z are > 0, and its three projected corners are finite.  The second
 *                   condition is deliberately narrower than the rasteriser's max z >= 0: a face that straddles the camera
 *                   plane has no meaningful outline.
 *   nearest point   c = the nearest point of the triangle's boundary to (px, py): over the edges (0,1), (0,2), (1,2) in this
 *                   order (a, b = the edge's corners), c_e = a + t (b - a), t = clamp(((b - a) . (p - a)) / |b - a|^2, 0, 1);
 *                   |b - a|^2 <= 1e-8: c_e = b and t = 1.  The first edge with the strictly smallest |c_e - p|^2 wins.
 *   signed distance inside <=> w0 > 0 and w1 > 0 and w2 > 0 (the barycentrics above);  d = |c - p|^2;  sd = -d inside, +d outside
 *   membership      f takes part AT p iff inside or d < r
 *   coverage        prob_f(p) = 1 / (1 + exp(sd / sigma));  trans_p = prod_f (1 - prob_f(p)) over the faces taking part at p,
 *                   multiplied in ascending face order starting from 1.0f;  alpha_p = 1 - trans_p.  A pixel no face takes part
 *                   at has trans = 1 and alpha = 0 exactly.
 * Two deviations from pytorch3d: every face near the pixel enters, there is no K-nearest cut (this is pytorch3d's result
 * whenever its faces_per_pixel is at least the overlap count); and the narrowed taking-part rule above.
 * Gradient, for an upstream gA [S*S]:   g_verts = d/dverts sum_p gA_p alpha_p        [V][3]
 * with membership, inside, the winning edge and a clamped t held constant:
 *   d alpha_p / d sd_f = -trans_p prob_f / sigma      (no division by 1 - prob_f: where the product is 0 the true value is 0 too)
 *   with s = -1 inside, +1 outside:  d sd / da = 2 s (1 - t)(c - p),  d sd / db = 2 s t (c - p)  (the clamped and the
 *   degenerate-edge cases included); the third corner gets 0.  NDC -> view -> world exactly as reni_gbuffer_backward
 *   (x = q_x / (q_z tan_half_fov), d/dp_i = sum_j R[i][j] d/dq_j).  The camera is a constant.
 * A vertex that no taking-part face names gets exactly 0.  Malformed input (an index outside [0, V), a list entry outside
 * [0, 3F), offsets outside their list) adds nothing and is never turned into an address.  fp32, no float atomics: every sum
 * and product has one fixed order, two calls give identical bits.
 * reni_soft_silhouette: R [9], T [3] (host memory) as reni_rasterize_mesh; alpha, trans [S*S] are overwritten.
 *   ws: reni_soft_silhouette_workspace_bytes(V, F, H, W) bytes, 256-byte aligned (the per-face records).
 * reni_soft_silhouette_backward: the same geometry arguments, sigma and blur_radius; trans [S*S] as the forward gave it;
 *   grad_alpha [S*S]; vf_offsets / vf_corners as for reni_mesh_vertex_normals; grad_verts [V][3] is overwritten.
 *   ws: reni_soft_silhouette_backward_workspace_bytes(V, F, H, W) bytes, 256-byte aligned (the records, 9 floats per face). */
size_t reni_soft_silhouette_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W);
int reni_soft_silhouette(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* R, const float* T,
                         float tan_half_fov, int64_t H, int64_t W, float sigma, float blur_radius, float* alpha, float* trans,
                         void* ws, size_t ws_bytes, void* stream);
size_t reni_soft_silhouette_backward_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W);
int reni_soft_silhouette_backward(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* R, const float* T,
                                  float tan_half_fov, int64_t H, int64_t W, float sigma, float blur_radius, const float* trans,
                                  const float* grad_alpha, const int64_t* vf_offsets, const int64_t* vf_corners,
                                  float* grad_verts, void* ws, size_t ws_bytes, void* stream);

/* ---- camera gradients of the G-buffer and of the soft silhouette: R, T and tan_half_fov (reni_tu_camera.hip) -------------
 * What the two backwards above hold constant: the pose.  With q = p R + T, t = tan_half_fov, x = q_x / (q_z t),
 * y = q_y / (q_z t) as above, let (tx_fk, ty_fk) be the gradient of the scalar objective with respect to the NDC position of
 * corner k of face f:
 *   soft silhouette   the corner's NDC sums of reni_soft_silhouette_backward (d sd / da, d sd / db over the face's pairs)
 *   G-buffer          the barycentric path alone: the corner's sums through the edge functions plus (d L / dA) dA / d(x, y)_k.
 *                     The vertex normals and the direct weights of X_p are world-space and do not see the camera.
 * Both kernels already form the view-space gradient of the corner, g_q = (tx / (z t), ty / (z t), -(tx x + ty y) / z).  Then,
 * with p_fk the corner's world position,
 *   gT[j]    = sum_{f,k} g_q,fk[j]
 *   gR[i][j] = sum_{f,k} p_fk[i] g_q,fk[j]          (row-major, R's own layout; R is differentiated as nine free numbers)
 *   g_tan    = -sum_{f,k} (tx_fk x_fk + ty_fk y_fk) / t
 * Held constant, as in the vertex gradients: the face assignment; membership, inside, the winning edge and a clamped t;
 * blur_radius and the grown boxes; 1e-8.  A face the forward skips, or one that does not take part, adds exactly 0.
 * grad_camera [13] (device) = gR [9], gT [3], g_tan [1], overwritten.  fp32, no float atomics: per face the three corners are
 * added in ascending order from 0, the faces are added by a store-then-sum reducer (chunks of 512 consecutive faces, a fixed
 * lane stride, a fixed butterfly, the waves in ascending order, then the same pass over the chunk sums until one is left)
 * whose order depends on F alone; two calls give identical bits.  Malformed input adds nothing and is never turned into an
 * address.
 * reni_gbuffer_backward_camera / reni_soft_silhouette_backward_camera: the arguments of reni_gbuffer_backward /
 *   reni_soft_silhouette_backward with grad_camera behind grad_verts.  grad_verts, when given, gets the bits of those entry
 *   points.  grad_verts, vf_offsets and vf_corners may be NULL together (the mesh is known, only the pose is fitted): the
 *   vertex kernels are then not launched and no list is needed.  grad_camera must not be NULL.
 *   ws: the _camera_workspace_bytes(V, F, H, W) of the entry point, 256-byte aligned. */
size_t reni_gbuffer_backward_camera_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W);
int reni_gbuffer_backward_camera(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* vert_normals,
                                 const float* R, const float* T, float tan_half_fov, int64_t H, int64_t W,
                                 const int64_t* pix_to_face, const int64_t* face_pixel_offsets, const int64_t* face_pixel_list,
                                 const int64_t* vf_offsets, const int64_t* vf_corners, const float* grad_pixel_normals,
                                 const float* grad_pixel_positions, float* grad_verts, float* grad_camera /* [13] device */,
                                 void* ws, size_t ws_bytes, void* stream);
size_t reni_soft_silhouette_backward_camera_workspace_bytes(int64_t V, int64_t F, int64_t H, int64_t W);
int reni_soft_silhouette_backward_camera(int64_t V, int64_t F, const float* verts, const int64_t* faces, const float* R,
                                         const float* T, float tan_half_fov, int64_t H, int64_t W, float sigma, float blur_radius,
                                         const float* trans, const float* grad_alpha, const int64_t* vf_offsets,
                                         const int64_t* vf_corners, float* grad_verts, float* grad_camera /* [13] device */,
                                         void* ws, size_t ws_bytes, void* stream);

/* ---- mesh regularisers: edge length, Laplacian smoothing, normal consistency (reni_tu_meshreg.hip) ------------------------
 * What keeps a fitted mesh a surface: the three terms of SoftRas / pytorch3d.loss (mesh_edge_loss, mesh_laplacian_smoothing,
 * mesh_normal_consistency) as ONE weighted objective  L = w_e L_e + w_l L_l + w_n L_n,  its three values and d L / d verts,
 * from one call.  Where pytorch3d differs from the text below, the text holds.
 * Topology.  A face TAKES PART iff its three indices lie in [0, V) and are pairwise different.  edges [E][2] are the unique
 *   undirected edges (a < b) of the faces taking part, in ascending (a, b).  The multiplicity of an edge is the number of
 *   faces taking part that hold it (a repeated face counts twice).  A PAIR is an unordered pair of faces on one edge: an edge
 *   of multiplicity m has m (m - 1) / 2 pairs, enumerated in ascending (edge, face, face); P is their number.
 * Edge loss.         L_e = (1 / E) sum_e (|x_a - x_b| - target_length)^2;  d|u| / du = 0 at u = 0;  E = 0 gives 0.
 * Laplacian, uniform (RENI_LAPLACIAN_UNIFORM).
 *                    r_v = mean_{j in N(v)} x_j - x_v over the unique neighbours of v;  L_l = (1 / V) sum_v |r_v|;
 *                    d|r| / dr = r / |r|, and 0 at r = 0.
 * Laplacian, cot (RENI_LAPLACIAN_COT).
 *                    With the side lengths A, B, C opposite corners 0, 1, 2 of a face, s = (A + B + C) / 2:
 *                    area = max(sqrt(max(s (s - A)(s - B)(s - C), 0)), 1e-12)  (Heron, clamped below at 1e-12);
 *                    cot_0 = (B^2 + C^2 - A^2) / (4 area), the other corners by the same pattern;
 *                    w_e = the sum over the edge's faces of the cotangent of the angle opposite the edge;
 *                    s_v = sum_j w_vj;  n_v = 1 / s_v if s_v > 0, else s_v;  r_v = (sum_j w_vj x_j) n_v - x_v.
 *                    The weights and n_v are CONSTANTS of the gradient (pytorch3d computes them without grad); they are
 *                    recomputed from the current vertices at every call.  "cotcurv" is not implemented.
 * Normal consistency.  For a pair on edge (a, b) with the opposite vertices c, d:
 *                    n0 = (x_b - x_a) x (x_c - x_a),  n1 = -(x_b - x_a) x (x_d - x_a),
 *                    cos = n0 . n1 / (max(|n0|, 1e-8) max(|n1|, 1e-8));  L_n = (1 / P) sum (1 - cos);  P = 0 gives 0.
 *                    Independent of the winding; a flat pair gives 0, a repeated face gives 2.  Where a max takes its floor,
 *                    the floor is a constant of the gradient.
 * Deviations from pytorch3d: a vertex WITHOUT NEIGHBOURS has r_v = 0 under either method (pytorch3d pulls it to the origin); it
 *   still counts in V.  The clamp of Heron's formula is on the area, not on the product under the root.  Faces with a
 *   repeated or out-of-range index take no part (pytorch3d has no such faces).
 * The lists (ops.mesh_edge_lists builds them once per face tensor; all int64, ascending; they depend on the faces alone):
 *   edges [E][2];  ef_offsets [E + 1] into ef_corners [H]: per edge the corners 3 f + k OPPOSITE it of the faces that hold it,
 *   ascending;  ve_offsets [V + 1] into ve_edges [2 E]: per vertex its edges, ascending;  vf_offsets [V + 1] into
 *   vf_corners [NC]: per vertex its corners (as for reni_mesh_vertex_normals);  corner_edges [3 F]: per corner the edge
 *   opposite it, -1 for a face that takes no part.  None of them is trusted: an offset is clamped into its list, an edge must
 *   be 0 <= a < b < V, an ef entry a corner of a face taking part whose opposite edge is that edge, a ve entry an edge that
 *   holds the vertex, a corner must name the vertex, corner_edges must agree with the face.  What fails adds nothing and is
 *   never turned into an address (a corner that an ef range repeats pairs with nothing).  An empty list is still a non-NULL
 *   pointer.  An edge of multiplicity m costs one thread m (m - 1) / 2 pairs; P must stay below 2^31 (a 32-bit count).
 * values [4] (device) = L, L_e, L_l, L_n, overwritten.  grad_verts [V][3] (device) = d L / d verts, overwritten; NULL: the
 *   values alone (the same bits).  A weight of 0 skips that loss's work: its value is 0 and it adds exactly 0.  Weights and
 *   target_length must be >= 0 and finite.
 * fp32, no float atomics and no in-launch ticket: per edge the pairs in ascending order, per vertex its edges then its corners in
 *   list order, and a store-then-sum reducer (chunks of 4096 rows, a fixed lane stride, a fixed butterfly, the waves in
 *   ascending order, relaunched on the chunk sums until one is left) whose order depends on V and E alone: two calls give
 *   identical bits.
 * ws: reni_mesh_regularizers_workspace_bytes(V, F, E) bytes, 256-byte aligned (0 for sizes out of range). */
#define RENI_LAPLACIAN_UNIFORM 0
#define RENI_LAPLACIAN_COT 1
size_t reni_mesh_regularizers_workspace_bytes(int64_t V, int64_t F, int64_t E);
int reni_mesh_regularizers(int64_t V, int64_t F, int64_t E, int64_t H, int64_t NC, const float* verts, const int64_t* faces,
                           const int64_t* edges, const int64_t* ef_offsets, const int64_t* ef_corners, const int64_t* ve_offsets,
                           const int64_t* ve_edges, const int64_t* vf_offsets, const int64_t* vf_corners,
                           const int64_t* corner_edges, float w_edge, float w_laplacian, float w_normal, float target_length,
                           int32_t method, float* values /* [4] device */, float* grad_verts /* [V][3] device, or NULL */,
                           void* ws, size_t ws_bytes, void* stream);

/* ---- point clouds: nearest points, the chamfer gradient, samples of a mesh's surface (reni_tu_points.hip) -----------------
 * What scores a recovered shape against the true one, and pulls a mesh towards a cloud: sample both surfaces, take the chamfer
 * distance and the F-score (reni_amd/mesh_losses.py).  fp32, no float atomics, no in-launch ticket, no host synchronisation,
 * launches on `stream` only: two calls give identical bits.  One cloud per call (no batches), no spatial index: brute force.
 *
 * reni_nearest_points.  For x [N][3], y [M][3]:  d(i, j) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with dx = x_i0 - y_j0, dy, dz
 *   likewise (exactly this form: the bits are defined).  idx[i] (int64) = the LOWEST j among those with the smallest d(i, j) as
 *   computed; dist2[i] = d(i, idx[i]).  The comparison is a strict <: where none succeeds (NaN coordinates, or every d = +inf),
 *   idx[i] = 0 and dist2[i] is what d(i, 0) computes.  A result is never turned into an address outside [0, M).
 *   Structure: 2 queries per lane in registers, 512 per workgroup; the targets pass through LDS in tiles of 1024 16-byte
 *   records that every lane reads at the same address.  grid.y cuts the target range into `slices` contiguous slices; with
 *   more than one, a second launch takes the lexicographic minimum of the slices' (d, j), so the result has the same bits for
 *   ANY slicing.  slices = 0: the library's choice, min(cap, ceil(M / 1024)); slices > 0 is clamped to min(cap, M), where
 *   cap = max(1, 512 / ceil(N / 512)) -- so slicing stops once the queries alone give 512 workgroups.
 *   Launches (counted by reni_launch_count): 1 with one slice, else 2.
 *   Limits: 1 <= N, M <= 2^31 - 1025.  ws: reni_nearest_points_workspace_bytes(N, M) bytes, 256-byte aligned (0 for sizes out of
 *   range): two 4-byte partials per (query, slice) for cap slices when cap > 1 -- at most 2 MiB + 256 bytes whatever N, and
 *   independent of M.  It is never N x M.
 *
 * reni_chamfer_grad.  For  L = (w_x / N) sum_i dist2_x[i] + (w_y / M) sum_j dist2_y[j]  with idx_xy [N] (x's nearest y) and
 *   idx_yx [M] (y's nearest x) from two searches, held CONSTANT:
 *     grad_x[i] = g (2 w_x / N) (x_i - y_idx_xy[i]) + g (2 w_y / M) sum_{j : idx_yx[j] = i} (x_i - y_j),
 *   evaluated as (g cx) t1 + (g cy) t2 with cx = (2 w_x) / N, cy = (2 w_y) / M in fp32; g is read from the device.  The second
 *   term is gathered through the sorted table (order [M] = the stable argsort of idx_yx, offsets [N + 1] = where each i's
 *   range starts; ops.chamfer_table) by reni_texture_fetch_backward's rule: a range of at most 128 entries is summed by its
 *   lane from 0 in order; a longer one in chunks of 64 consecutive entries by the 64 lanes of the wave (lane l adds entries
 *   l, l + 64, ...), combined by the xor butterfly 32, 16, 8, 4, 2, 1.  An idx_xy entry or an order entry outside [0, M) adds
 *   nothing, offsets are clamped into [0, M]: nothing of them is trusted as an address.  A weight of 0 skips its term, which
 *   adds exactly 0, and its lists may be NULL.  Weights must be >= 0 and finite.  Called with the roles swapped it gives
 *   grad_y.  grad_x [N][3] is overwritten.  1 launch.
 *
 * reni_mesh_sample_table.  table [2][F] (device): table[0][f] = the area of face f, 0.5 |(x_1 - x_0) x (x_2 - x_0)| in fp32; a
 *   face that does not TAKE PART (the regularisers' rule: indices in [0, V), pairwise different) and an area that is 0 or not
 *   finite count as 0.  table[1][f] = the CDF: the inclusive prefix sums of the areas in double by a parallel scan in a fixed
 *   order (Hillis-Steele in a wave, waves, 256-entry tiles and 1024-face chunks in ascending order), divided by the scan's own
 *   value at the last chunk with mass and rounded once; made ascending, and flat over a face without area, by a running
 *   maximum behind the division, as reni_light_table_build's CDFs are.  The last face with area and everything behind it hold
 *   exactly 1.0f.  Total area 0: the CDF is 0 everywhere.  3 launches.  ws: reni_mesh_sample_table_workspace_bytes(F).
 *
 * reni_mesh_sample_points.  For u [S][3] (each clamped into [0, 1), NaN -> 0):  face = the number of CDF entries <= u0, at most
 *   F - 1 -- a face without area is never chosen;  r = sqrtf(u1),  w = (1 - r, r (1 - u2), r u2)  (pytorch3d's).  The output is
 *   a tap table of the texture unit: tap_index [S][8] int32 = the face's three vertices then 0, tap_weight [S][8] = w then 0;
 *   and face_idx [S] int64.  Positions are reni_texture_fetch(P = S, E = V, C = 3, tex = verts) and the gradient with respect to
 *   the vertices is reni_texture_fetch_backward: the face choice and the barycentrics are CONSTANTS of the gradient.  A table
 *   without mass (its last CDF entry is not 1.0f) gives all-zero weights and index 0, so the points are exactly 0; no host
 *   check.  tap_index and tap_weight must be 16-byte aligned for the fetch.  1 launch.  Limits: V, F < 2^30, S < 2^28. */
size_t reni_nearest_points_workspace_bytes(int64_t N, int64_t M);
int reni_nearest_points(int64_t N, int64_t M, const float* x, const float* y, int32_t slices, float* dist2 /* [N] */,
                        int64_t* idx /* [N] */, void* ws, size_t ws_bytes, void* stream);
int reni_chamfer_grad(int64_t N, int64_t M, const float* x, const float* y, const int64_t* idx_xy /* [N], or NULL with w_x = 0 */,
                      const int64_t* order /* [M] */, const int64_t* offsets /* [N + 1]; both may be NULL with w_y = 0 */,
                      float w_x, float w_y, const float* g /* [1] device */, float* grad_x /* [N][3] */, void* stream);
size_t reni_mesh_sample_table_workspace_bytes(int64_t F);
int reni_mesh_sample_table(int64_t V, int64_t F, const float* verts, const int64_t* faces, float* table /* [2][F] */, void* ws,
                           size_t ws_bytes, void* stream);
int reni_mesh_sample_points(int64_t V, int64_t F, int64_t S, const int64_t* faces, const float* table, const float* u /* [S][3] */,
                            int32_t* tap_index /* [S][8] */, float* tap_weight /* [S][8] */, int64_t* face_idx /* [S] */,
                            void* stream);

/* ---- points against a mesh: the nearest triangle of a point, the nearest point of a triangle (reni_tu_pointmesh.hip) -------
 * What the sample-based scores above cannot give: the distance from a point to the SURFACE (pytorch3d's
 * point_mesh_face_distance, both directions), so a mesh scored against itself scores 0 and a scan pulls on the surface
 * itself (reni_amd/mesh_losses.py: nearest_surface, point_mesh_distance, geometry_scores(surface=True)).  fp32, no float
 * atomics, no in-launch ticket, no host synchronisation, launches on `stream` only: two calls give identical bits.  One mesh
 * and one cloud per call, no spatial index and no culling: brute force.
 *
 * The pair function.  For a point p and the triangle (a, b, c), every operation in fp32, none contracted, dot(u, v) =
 * fmaf(u2, v2, fmaf(u1, v1, u0 * v0)):
 *     ab = b - a, ac = c - a;  ap = p - a, bp = ap - ab, cp = ap - ac;
 *     d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
 *     vc = fmaf(d1, d4, -(d3 * d2)), vb = fmaf(d5, d2, -(d1 * d6)), va = fmaf(d3, d6, -(d5 * d4));
 *   the FIRST of these regions that holds gives (nv, nw, den):
 *     vertex a:  d1 <= 0 and d2 <= 0                          (0, 0, 1)
 *     vertex b:  d3 >= 0 and d4 <= d3                         (1, 0, 1)
 *     edge ab:   vc <= 0 and d1 >= 0 and d3 <= 0              (d1, 0, d1 - d3)
 *     vertex c:  d6 >= 0 and d5 <= d6                         (0, 1, 1)
 *     edge ac:   vb <= 0 and d2 >= 0 and d6 <= 0              (0, d2, d2 - d6)
 *     edge bc:   va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    (d5 - d6, d4 - d3, (d4 - d3) + (d5 - d6))
 *     interior:                                               (vb, vc, (va + vb) + vc)
 *   r = 1 / den (correctly rounded);  v = min(max(nv r, 0), 1);  w = min(max(nw r, 0), 1 - v)  with fmaxf / fminf, so a NaN
 *   quotient (0 / 0: a triangle without area) becomes 0.  The weights are (u, v, w) with u = (1 - v) - w: every one is >= 0
 *   and they sum to 1, so q = a + v ab + w ac, evaluated as fmaf(w, ac, fmaf(v, ab, a)) per component, is a point of the
 *   triangle.  d = fmaf(rz, rz, fmaf(ry, ry, rx * rx)) with r = p - q.  A vertex that is not finite makes q, and so d, a NaN.
 *   A face TAKES PART by the regularisers' rule: indices in [0, V), pairwise different.  A face that takes no part is
 *   compared as NaN.  Every comparison is a strict <, so a NaN and a face that takes no part win none.
 *
 * reni_nearest_faces.  For points [N][3], verts [V][3], faces [F][3] (int64):  face_idx[i] (int64) = the LOWEST f among those
 *   with the smallest d(p_i, f) as computed, dist2[i] = that d, and a tap row of the texture unit as reni_mesh_sample_points
 *   writes it: tap_index [N][8] int32 = the face's three vertices then 0, tap_weight [N][8] = (u, v, w) then 0.  The closest
 *   points are reni_texture_fetch(P = N, E = V, C = 3, tex = verts) (u a + v b + w c by its fmaf chain: the same point up to
 *   rounding) and reni_texture_fetch_backward carries their gradient to the vertices.  Where no face wins: face_idx = -1,
 *   dist2 = +inf, all-zero taps at index 0.  A result is never turned into an address outside [0, V) or [0, F).
 * reni_faces_nearest_points.  The other direction: point_idx[f] (int64) = the LOWEST i among those with the smallest
 *   d(p_i, f), dist2[f] = that d, and the tap row [F][8] of the closest point of face f to that p_i.  A face that takes no
 *   part, or against which no point wins: -1, +inf, zero taps.
 * Structure (both: one templated kernel, two instances): 2 queries per lane in registers, 512 per workgroup; the targets pass
 *   through LDS in tiles of 256 records that every lane reads at the same address -- a triangle as (a, ab, ac) in three
 *   16-byte words, prepared once per tile, or a point in one.  grid.y cuts the target range into `slices` contiguous slices;
 *   with more than one, a second launch takes the lexicographic minimum of the slices' (d, j), so the result has the same bits
 *   for ANY slicing.  slices = 0: the library's choice, min(cap, ceil(targets / 256)); slices > 0 is clamped to
 *   min(cap, targets), where cap = max(1, 512 / ceil(queries / 512)).  The tap row is computed from the winning pair by the
 *   pair function once more: the same bits.
 *   Launches (counted by reni_launch_count): 1 with one slice, else 2.
 *   Limits: 1 <= N, F <= 2^31 - 257, 1 <= V < 2^30; tap_index and tap_weight 16-byte aligned.  ws:
 *   reni_*_workspace_bytes(N, V, F) bytes, 256-byte aligned (0 for sizes out of range): two 4-byte partials per (query, slice)
 *   for cap slices when cap > 1 -- at most 2 MiB + 768 bytes, independent of the number of targets.  It is never N x F. */
size_t reni_nearest_faces_workspace_bytes(int64_t N, int64_t V, int64_t F);
int reni_nearest_faces(int64_t N, int64_t V, int64_t F, const float* points, const float* verts, const int64_t* faces, int32_t slices,
                       float* dist2 /* [N] */, int64_t* face_idx /* [N] */, int32_t* tap_index /* [N][8] */,
                       float* tap_weight /* [N][8] */, void* ws, size_t ws_bytes, void* stream);
size_t reni_faces_nearest_points_workspace_bytes(int64_t N, int64_t V, int64_t F);
int reni_faces_nearest_points(int64_t N, int64_t V, int64_t F, const float* points, const float* verts, const int64_t* faces,
                              int32_t slices, float* dist2 /* [F] */, int64_t* point_idx /* [F] */, int32_t* tap_index /* [F][8] */,
                              float* tap_weight /* [F][8] */, void* ws, size_t ws_bytes, void* stream);

/* ---- cloud neighbourhoods: the K nearest points, normals from their principal axes (reni_tu_knn.hip) ---------------------
 * What lets a scan pull on ORIENTATION and scores normal consistency: a scan arrives without normals, they are estimated from
 * the K nearest neighbours of every point (pytorch3d's knn_points and estimate_pointcloud_normals; reni_amd/mesh_losses.py:
 * knn_points, estimate_normals, chamfer_distance(x_normals=, y_normals=), geometry_scores(normals=True)).  fp32, no float
 * atomics, no in-launch ticket, no host synchronisation, launches on `stream` only: two calls give identical bits.  One cloud
 * per call, no spatial index: brute force, never N x M.
 *
 * reni_knn_points.  d(i, j) is reni_nearest_points' expression, fmaf(dz, dz, fmaf(dy, dy, dx * dx)), uncontracted.  Row i of
 *   dist2 [N][K] (float32) and idx [N][K] (int64) lists the K smallest pairs (d, j) in ascending LEXICOGRAPHIC order: ties in d
 *   go by ascending j.  A j whose d is NaN or +inf is never listed.  Slots left unfilled (M < K, a NaN query, every distance
 *   overflowing) hold +inf and -1.  No index outside [-1, M) is ever written.  Column 0 has reni_nearest_points' bits wherever
 *   slot 0 is filled.  1 <= K <= 32.
 *   Structure: ONE query per lane, 256 per workgroup, its list of KB pairs in registers, KB the next of {4, 8, 16, 32} at or
 *   above K (a smaller K runs in that bucket and stores its first K slots); the targets pass through LDS in tiles of 1024
 *   16-byte records that every lane reads at the same address.  Per target one comparison against the lane's last slot; the
 *   fully unrolled insertion runs only where a wave ballot says some lane improved.  grid.y cuts the target range into `slices`
 *   contiguous slices; with more than one, a second launch merges the slices' lists lexicographically, so the result has the
 *   same bits for ANY slicing.  slices = 0: the library's choice, min(cap, ceil(M / 1024)); slices > 0 is clamped to
 *   min(cap, M), where cap = max(1, 512 / ceil(N / 256)) -- reni_nearest_points' rule for 256 queries per workgroup.
 *   Launches (counted by reni_launch_count): 1 with one slice, else 2.
 *   Limits: 1 <= N, M <= 2^31 - 1025.  ws: reni_knn_points_workspace_bytes(N, M, K) bytes, 256-byte aligned (0 for sizes or a K
 *   out of range): the partials, cap N K pairs of two 4-byte values when cap > 1 -- N cap <= 131072, so at most K MiB + 768
 *   bytes whatever N, and independent of M.
 *
 * reni_cloud_normals.  For y [M][3] and neighbour lists idx [N][K] (reni_knn_points' format), one lane per row, in fp32 with no
 *   contraction, in THIS order:
 *     mean:     s = 0; for the slots k = 0 .. K - 1 in list order, skipping a slot that is -1 or outside [0, M): s += y_j,
 *               per component; c = the number of slots used; m = s / c.
 *     moments:  for the same slots in the same order, e = y_j - m:  Cxx = fmaf(ex, ex, Cxx), Cxy = fmaf(ex, ey, Cxy), Cxz, Cyy,
 *               Cyz, Czz likewise from 0; each divided by c.
 *     solve:    cyclic Jacobi on the symmetric 3 x 3 matrix, 6 sweeps of the rotations (0,1), (0,2), (1,2); a rotation (p, q)
 *               with a_pq != 0:  theta = (a_qq - a_pp) / (2 a_pq),  t = copysign(1, theta) / (|theta| + sqrt(fmaf(theta, theta,
 *               1))),  c = 1 / sqrt(fmaf(t, t, 1)),  s = t c;  a_pp -= t a_pq, a_qq += t a_pq, a_pq = 0, the third row r:
 *               (a_rp, a_rq) <- (c a_rp - s a_rq, s a_rp + c a_rq); the columns p, q of V (from the identity) likewise.
 *     eigenvalues [N][3] = the diagonal, ASCENDING (three compare-exchanges that carry V's columns), clamped at 0 from below.
 *     normals [N][3] = V's column of the smallest eigenvalue divided by its length: a unit vector.
 *   Sign.  With viewpoint ([3], device): row i is point y_i (needs N <= M) and the normal is negated where
 *   n . (viewpoint - y_i) < 0, so n . (viewpoint - y_i) >= 0.  With viewpoint = NULL: the component of largest magnitude is
 *   made positive, the lowest index on ties.
 *   Degenerate.  Fewer than 3 usable slots: normal exactly (0, 0, 0), eigenvalues 0.  A neighbourhood on a line or in a point:
 *   some finite unit vector orthogonal to the rest (coincident points: (1, 0, 0)).  Moments that are not finite: (0, 0, 1),
 *   eigenvalues clamped (NaN -> 0).  Never a NaN.  1 launch. */
size_t reni_knn_points_workspace_bytes(int64_t N, int64_t M, int64_t K);
int reni_knn_points(int64_t N, int64_t M, int64_t K, const float* x, const float* y, int32_t slices, float* dist2 /* [N][K] */,
                    int64_t* idx /* [N][K] */, void* ws, size_t ws_bytes, void* stream);
int reni_cloud_normals(int64_t N, int64_t M, int64_t K, const float* y, const int64_t* idx /* [N][K] */,
                       const float* viewpoint /* [3] device, or NULL */, float* normals /* [N][3] */,
                       float* eigenvalues /* [N][3] */, void* stream);

/* ---- cast shadows: visibility masks of the mesh for the shader (reni_tu_visibility.hip, the MASKED shader instances) ----
 * The shader above lets light pass through the mesh: M(p, j) knows the pixel's own normal and nothing else.  The lights are at
 * infinity, so whether texel direction j reaches pixel p is a constant of (mesh, camera, directions), as the G-buffer is.
 * Definition.  Pixel p has the origin o = pixel_positions[p] and its own face pix_to_face[p]; d is a unit direction; face f has
 * the vertices v0, v1, v2 (a face with an index outside [0, V) is skipped, as in the rasteriser):
 *     e1 = v1 - v0, e2 = v2 - v0, h = d x e2, a = e1 . h;          |a| <= 1e-12: miss
 *     s = o - v0, u = (s . h) / a, q = s x e1, v = (d . q) / a, t = (e2 . q) / a
 *     hit  <=>  f != own face  and  u >= 0  and  v >= 0  and  u + v <= 1  and  t > t_min
 *   Two-sided, no culling (as the rasteriser).  Bit (p, j) is 1 ("visible") iff no face hits; a background pixel
 *   (pix_to_face < 0) has every bit 0.  fp32; the pass is deterministic (an any-hit query: two calls give identical bits).
 *   vis : uint32 [NB][NP][JW], JW = ceil(J / 32); bit j & 31 of word j >> 5; bits at j >= J are 0.  NB = 1 when the directions
 *         are shared (dirs_batch_stride == 0), else NB = B.
 * reni_mesh_visibility_prepare: the acceleration record of (verts [V][3], faces [F][3] int64) in the caller's buffer accel
 *   (reni_mesh_visibility_accel_bytes(F) bytes, 16-byte aligned; 0 for an F outside [1, 2^30)): per slot k the face order[k]
 *   (order [F] int64, a permutation that puts nearby faces next to each other, e.g. the argsort of the centroids' Morton codes;
 *   NULL: the given order) as v0, e1, e2 and its id, and one bounding box per cluster of 64 consecutive slots, grown by 2^-10 of
 *   its extent and position so that the fp32 slab test stays conservative.  The record is opaque and holds no pointer.
 * reni_mesh_visibility: positions [NP][3], pix_to_face [NP] int64 (the rasteriser's), dirs [J][3] of image b at
 *   dirs + b * dirs_batch_stride (floats; 0 = shared), 0 <= t_min finite (hits nearer than this are the surface itself).
 *   flags: RENI_VIS_NO_CULL visits every cluster of every ray (no box test, no early exit): brute force, the same bits.
 *   d need not be a unit vector: the formulas are evaluated as they stand (t scales by 1 / |d|).  A direction that is zero or
 *   has a NaN or infinite component hits no face (a is 0 or NaN, or u and v are NaN): its bit is 1 on every foreground pixel.
 *   An accel buffer that reni_mesh_visibility_prepare never filled (no magic number in its first word) is not walked: it
 *   stands for a mesh without faces, foreground bits 1, background bits 0; nothing beyond its 64-byte header is read.  A
 *   pix_to_face that is no face's id (>= F, or the id of a skipped face) excludes nothing. */
#define RENI_VIS_NO_CULL 1u
size_t reni_mesh_visibility_accel_bytes(int64_t F);
int reni_mesh_visibility_prepare(int64_t V, int64_t F, const float* verts, const int64_t* faces, const int64_t* order,
                                 void* accel, size_t accel_bytes, void* stream);
int reni_mesh_visibility(int64_t B, int64_t NP, int64_t J, const float* positions, const int64_t* pix_to_face,
                         const float* dirs, int64_t dirs_batch_stride, const void* accel, float t_min, uint32_t flags,
                         uint32_t* vis, void* stream);
/* The shader with a mask: colors[b,p] = sum_j vis(p,j) M(p,j) C[b,j], dC[b,j] = sum_p vis(p,j) M(p,j) dcolors[b,p]; every other
 * argument, the workspace, the splits and the summation order are reni_envmap_shade's, so an all-ones mask gives its bits.
 *   vis : [NB][NP][ceil(J/32)] as above, image b's at vis + b * vis_batch_stride (words; 0 = one mask for all images, required
 *         when dirs_batch_stride == 0). */
int reni_envmap_shade_masked(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                             float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                             const float* light_colors, float shininess, float kd, float ks, const uint32_t* vis,
                             int64_t vis_batch_stride, float* colors, void* ws, size_t ws_bytes, void* stream);
int reni_envmap_shade_masked_backward(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions,
                                      float cam_x, float cam_y, float cam_z, const float* light_dirs,
                                      int64_t dirs_batch_stride, const float* dcolors, float shininess, float kd, float ks,
                                      const uint32_t* vis, int64_t vis_batch_stride, float* dlight_colors, void* ws,
                                      size_t ws_bytes, void* stream);

/* ---- per-pixel materials: the shader's terms, for an albedo, a ks and a shininess per pixel and their gradients ----
 * With nl, nh as in reni_envmap_shade (nl = clamp(N.L, 0, 1), nh = clamp(N.normalize(V + L), 0, 1)), s_p the pixel's
 * shininess and v(p,j) the visibility bit (1 when vis is NULL):
 *     diffuse[b,p,:]      = sum_j v nl                C[b,j,:]
 *     specular[b,p,:]     = sum_j v nh^s_p            C[b,j,:]     (no norm(s), no ks: the caller applies the material,
 *                                                                   colors = albedo diffuse + ks norm(s_p) specular)
 *     dspecular_ds[b,p,:] = sum_j v nh^s_p ln nh      C[b,j,:]     (d specular / d s_p; a pair with nh = 0 adds exactly 0;
 *                                                                   NULL: not wanted, not computed)
 *     dlight_colors[b,j,:] = sum_p v ( nl d_diffuse[b,p,:] + nh^s_p d_specular[b,p,:] )
 * normals .. light_colors, vis, vis_batch_stride: as for reni_envmap_shade[_masked]; the three outputs and the two upstream
 * gradients are [B][NP][3].  shininess: device, s_p = shininess[p * shininess_stride], shininess_stride 0 (one value for all
 * pixels) or 1 ([NP]).  Every s_p must be > 0: a value <= 0 or NaN gives unspecified values for that pixel (and, backward,
 * for the texels it lights), never an access outside the buffers.  Deterministic (fixed-order partial sums, no float
 * atomics); an all-ones mask gives the bits of vis = NULL.
 * ws: reni_envmap_shade_terms_workspace_bytes(B, NP, J, flags) bytes, flags = RENI_SHADE_TERMS_DS when dspecular_ds is
 * wanted, else 0 (0 is returned for a size < 1 or an unknown flag); one buffer of that size serves both calls. */
#define RENI_SHADE_TERMS_DS 1u
size_t reni_envmap_shade_terms_workspace_bytes(int64_t B, int64_t NP, int64_t J, uint32_t flags);
int reni_envmap_shade_terms(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                            float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                            const float* light_colors, const float* shininess, int64_t shininess_stride, const uint32_t* vis,
                            int64_t vis_batch_stride, float* diffuse, float* specular, float* dspecular_ds, void* ws,
                            size_t ws_bytes, void* stream);
int reni_envmap_shade_terms_backward(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions,
                                     float cam_x, float cam_y, float cam_z, const float* light_dirs,
                                     int64_t dirs_batch_stride, const float* shininess, int64_t shininess_stride,
                                     const uint32_t* vis, int64_t vis_batch_stride, const float* d_diffuse,
                                     const float* d_specular, float* dlight_colors, void* ws, size_t ws_bytes, void* stream);
/* Normal-mapped materials: d loss / d normals of the two sums above, for upstream gradients d_diffuse, d_specular.  With
 * n_p the given normal, N = n_p / max(|n_p|, 1e-6), H = normalize(V + L), x_l = N.L and x_h = N.H (before their clamps),
 * a(b,p,j) = sum_c d_diffuse[b,p,c] C[b,j,c] and b'(b,p,j) = sum_c d_specular[b,p,c] C[b,j,c]:
 *     gN[p]        = sum_b sum_j v ( [x_l > 0] a L_j + [x_h > 0] s_p nh^(s_p - 1) b' H )
 *     d_normals[p] = (gN - N (N.gN)) / |n_p|  for |n_p| >= 1e-6,  gN / 1e-6 below it (F.normalize's eps branch)
 * The gates are strict and the clamps at 1 are ignored (x <= 1, and at x = 1 the projection removes the term); a pixel with
 * a zero normal (background) gets exactly 0 -- torch autograd on a zero normal gives L a / 1e-6 instead, clamp's backward
 * passing the boundary.  Arguments as for reni_envmap_shade_terms; d_normals is [NP][3].  Each image has its own L when
 * dirs_batch_stride != 0; the sum over images is taken in image order.  s_p <= 0 or NaN gives unspecified values for that
 * pixel only, never an access outside the buffers.  Deterministic (fixed-order partial sums, no float atomics); an
 * all-ones mask gives the bits of vis = NULL.
 * ws: reni_envmap_shade_terms_dnormals_workspace_bytes(B, NP, J) bytes (0 is returned for a size < 1); always needed. */
size_t reni_envmap_shade_terms_dnormals_workspace_bytes(int64_t B, int64_t NP, int64_t J);
int reni_envmap_shade_terms_dnormals(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions,
                                     float cam_x, float cam_y, float cam_z, const float* light_dirs,
                                     int64_t dirs_batch_stride, const float* light_colors, const float* shininess,
                                     int64_t shininess_stride, const uint32_t* vis, int64_t vis_batch_stride,
                                     const float* d_diffuse, const float* d_specular, float* d_normals, void* ws,
                                     size_t ws_bytes, void* stream);

/* ---- microfacet (GGX) materials: the shader's terms for a base colour / roughness / metallic surface ------------------
 * For pixel p with given normal n_p: N = n_p / max(|n_p|, 1e-6), V = normalize(cam - pos_p), a = alpha_p > 0.  For texel j
 * with direction L, colour C[b,j,:] and visibility bit v(p,j) (1 when vis is NULL):
 *     H   = (V + L) / max(|V + L|, 1e-6)
 *     x_l = N.L,  x_h = N.H,  x_v = N.V            nl, nh, nv = clamp(x, 0, 1)
 *     u   = clamp(V.H, 0, 1)                        f = (1 - u)^5
 *     s2  = |N x H|^2                               (= 1 - x_h^2 for unit vectors, without the cancellation at the lobe's peak)
 *     d   = a^2 nh^2 + s2
 *     lam(x) = sqrt(a^2 + (1 - a^2) x^2)
 *     k   = [x_h > 0] a^2 nl / ( d^2 (nl + lam(nl)) (nv + lam(nv)) )
 *
 *     diffuse[b,p,c] = sum_j v nl  C[b,j,c]         (reni_envmap_shade_terms' diffuse sum, bit for bit)
 *     spec0 [b,p,c]  = sum_j v k   C[b,j,c]
 *     spec1 [b,p,c]  = sum_j v k f C[b,j,c]
 *     dlight_colors[b,j,c] = sum_p v ( nl d_diffuse[b,p,c] + k d_spec0[b,p,c] + k f d_spec1[b,p,c] )
 *     d_alpha[p]     = sum_b sum_j v (dk/da) ( sum_c d_spec0 C + f sum_c d_spec1 C )
 *     d_normals[p]   = Jacobian of F.normalize applied to sum_b sum_j v ( [x_l > 0] (sum_c d_diffuse C) L + the d(k, k f)/dN
 *                      terms ), with strict gates and the projection as in reni_envmap_shade_terms_dnormals
 * k is the GGX distribution times the separable Smith visibility times nl, without 1 / pi (the diffuse sum carries none
 * either: both are pi times the physical radiance).  Schlick's Fresnel is affine in F0, so the caller composes
 * colours = (1 - metallic) base_color diffuse + F0 spec0 + (1 - F0) spec1.  Every denominator is at least a power of a: no
 * epsilon; a pair with nl = 0 adds exactly 0; a pixel with a zero normal gets exact zeros in every output and gradient.
 * normals .. light_colors, vis, vis_batch_stride: as for reni_envmap_shade_terms.  alpha: device, a_p = alpha[p * alpha_stride],
 * alpha_stride 0 (one value for all pixels) or 1 ([NP]).  a_p <= 0 or NaN gives unspecified values for that pixel (backward:
 * for the texels it lights), never an access outside the buffers.  d_alpha is [NP] at either stride (stride 0: the caller
 * sums it); d_normals [NP][3] or NULL (not wanted, not computed: d_alpha keeps its bits).  Deterministic (fixed-order partial
 * sums, no float atomics); an all-ones mask gives the bits of vis = NULL.
 * ws: reni_envmap_shade_ggx_workspace_bytes(B, NP, J) serves the forward and the backward call,
 * reni_envmap_shade_ggx_dpixel_workspace_bytes(B, NP, J) the dpixel call, which always needs it (0 for a size < 1). */
size_t reni_envmap_shade_ggx_workspace_bytes(int64_t B, int64_t NP, int64_t J);
int reni_envmap_shade_ggx(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                          float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                          const float* light_colors, const float* alpha, int64_t alpha_stride, const uint32_t* vis,
                          int64_t vis_batch_stride, float* diffuse, float* spec0, float* spec1, void* ws, size_t ws_bytes,
                          void* stream);
int reni_envmap_shade_ggx_backward(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                                   float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                                   const float* alpha, int64_t alpha_stride, const uint32_t* vis, int64_t vis_batch_stride,
                                   const float* d_diffuse, const float* d_spec0, const float* d_spec1, float* dlight_colors,
                                   void* ws, size_t ws_bytes, void* stream);
size_t reni_envmap_shade_ggx_dpixel_workspace_bytes(int64_t B, int64_t NP, int64_t J);
int reni_envmap_shade_ggx_dpixel(int64_t B, int64_t NP, int64_t J, const float* normals, const float* positions, float cam_x,
                                 float cam_y, float cam_z, const float* light_dirs, int64_t dirs_batch_stride,
                                 const float* light_colors, const float* alpha, int64_t alpha_stride, const uint32_t* vis,
                                 int64_t vis_batch_stride, const float* d_diffuse, const float* d_spec0, const float* d_spec1,
                                 float* d_alpha, float* d_normals, void* ws, size_t ws_bytes, void* stream);

/* ---- environment-map baselines: spherical Gaussians and spherical harmonics ----------------------------------------
 * What RENI is compared against.  fp32, deterministic (no float atomics; fixed summation order: two calls give identical
 * bits, and map n's results are the same alone or inside a batch).
 * Spherical Gaussians, SGEnvOptim (src/models/spherical_gaussians.py).  N >= 1 maps of H x W >= 1 pixels, 1 <= K <= 64 lobes.
 *   params [N][K][6] raw = (w0, w1, w2, theta~, phi~, lambda~) per lobe k = row * SGCol + col; theta_c / phi_c [K] the lobe centres
 *   (float32 of the reference's float64 meshgrid, :29-37); theta_range / phi_range the scalars of :38-39.  Lobe: theta = theta_range
 *   tanh theta~ + theta_c, phi = phi_range tanh phi~ + phi_c, w = exp w~, lambda = exp lambda~, axis a = (sin theta cos phi,
 *   sin theta sin phi, cos theta).  Pixel p = i W + j looks along l = (sin El cos Az, sin El sin Az, cos El), Az = ((j + 0.5) / W - 0.5)
 *   2 pi, El = (i + 0.5) / H pi / 2 (a hemisphere, :41-52).
 * reni_sg_render: rec [N][3][H][W] = sum_k w_kc exp(lambda_k (a_k . l_p - 1))                           (renderSG :109-137)
 * reni_sg_loss_grad: log_target [N][3][H][W] = log(env + 1); weight s at weight[n sn + c sc + i sh + j sw] (stride 0 broadcasts).
 *   loss_per_map [N] = mean over (c, p) of s (log(rec + 1) - log_target)^2; loss_total [1] their sum (WeightedMSE,
 *   loss_functions.py:6-13); dparams [N][K][6] = d loss_total / d params.  ws: reni_sg_workspace_bytes(N, K, H, W) bytes, 256-byte
 *   aligned (0 bytes -- ws may be NULL -- when H W <= 768). */
size_t reni_sg_workspace_bytes(int64_t N, int64_t K, int64_t H, int64_t W);
int reni_sg_render(int64_t N, int64_t K, int64_t H, int64_t W, const float* params, const float* theta_c, const float* phi_c,
                   float theta_range, float phi_range, float* rec, void* stream);
int reni_sg_loss_grad(int64_t N, int64_t K, int64_t H, int64_t W, const float* params, const float* theta_c, const float* phi_c,
                      float theta_range, float phi_range, const float* log_target, const float* weight, int64_t w_stride_n,
                      int64_t w_stride_c, int64_t w_stride_h, int64_t w_stride_w, float* loss_per_map, float* loss_total,
                      float* dparams, void* ws, size_t ws_bytes, void* stream);
/* Spherical harmonics (src/models/spherical_harmonics.py).  Equirectangular [N][H][W][3] maps, W even, H == W / 2, W <= 4096,
 * 0 <= lmax <= 15, T = (lmax + 1)^2 terms, t = l^2 + l + m.  Y_t(y, x) = row_table[y][t] col_table[x][t]: row_table [H][T] =
 * K_l|m| P_l|m|(cos(y pi / H)) (times sqrt 2 for m != 0), col_table [W][T] = cos(m x 2 pi / W) (m > 0), 1 (m = 0), sin(|m| x 2 pi / W)
 * (m < 0) -- the pixel's top-left corner, as getCoefficientsMatrix.  For the projection the caller folds the solid angle of row y,
 * 2 pi / W (cos(theta - pi / 2H) - cos(theta + pi / 2H)), theta = (1 - (y + 0.5) / H) pi (getSolidAngle), into row_table.
 * reni_sh_project: coeffs [N][T][3] = sum_(y, x) img[n][y][x][c] row_table[y][t] col_table[x][t]       (getCoefficientsFromImage)
 * reni_sh_reconstruct: out [N][H][W][3] = sum_t row_table[y][t] col_table[x][t] coeffs[n][t][c]         (shReconstructSignal) */
int reni_sh_project(int64_t N, int64_t H, int64_t W, int64_t lmax, const float* img, const float* row_table,
                    const float* col_table, float* coeffs, void* stream);
int reni_sh_reconstruct(int64_t N, int64_t H, int64_t W, int64_t lmax, const float* coeffs, const float* row_table,
                        const float* col_table, float* out, void* stream);

/* ---- diffuse irradiance (src/models/spherical_harmonics.py: getDiffuseMap, shRenderL2) --------------------------------
 * fp32, deterministic (no float atomics; fixed summation order that depends on (P, Q) only: two calls give identical bits,
 * and map n's results are the same alone or inside a batch).
 * reni_diffuse_convolve: out [N][P][3] = scale sum_(i < Q) max(0, out_dirs[o] . in_dirs[i]) in_w[i] src(n, i, c), the
 *   clamped-cosine convolution (getDiffuseMap :383-437 with scale = 1 / pi).  out_dirs [P][3], in_dirs [Q][3], in_w [Q] are
 *   shared by the N maps; src(n, i, c) = src[n src_stride_n + i src_stride_i + c src_stride_c] (element strides >= 0:
 *   [N][Q][3] is (3 Q, 3, 1), channel-planar [N][3][Q] is (3 Q, 1, Q)).  N, P, Q >= 1, 3 N P and 3 Q < 2^30.
 *   ws: reni_diffuse_workspace_bytes(N, P, Q) bytes, 256-byte aligned (0 bytes -- ws may be NULL -- when the i range is not
 *   split, which the library decides from (P, Q)).
 * reni_sh_irradiance_l2: out [N][P][3] = shRenderL2(coeffs[n], normal) (Ramamoorthi & Hanrahan 2001, the reference's C1..C5,
 *   its - C5 L6 term and its final / pi) for coeffs [N][9][3] and normal (x, y, z) = normals[n normals_stride_n + 3 p + 0..2];
 *   normals_stride_n is 0 (normals [P][3] shared) or 3 P (normals [N][P][3] per map). */
size_t reni_diffuse_workspace_bytes(int64_t N, int64_t P, int64_t Q);
int reni_diffuse_convolve(int64_t N, int64_t P, int64_t Q, const float* out_dirs, const float* in_dirs, const float* in_w,
                          const float* src, int64_t src_stride_n, int64_t src_stride_i, int64_t src_stride_c, float scale,
                          float* out, void* ws, size_t ws_bytes, void* stream);
int reni_sh_irradiance_l2(int64_t N, int64_t P, const float* coeffs, const float* normals, int64_t normals_stride_n, float* out,
                          void* stream);

/* ---- glossy lighting: zonal-lobe convolution and lookup at arbitrary directions (reni_tu_glossy.hip; reni_amd/glossy.py) ----
 * No reference counterpart.  fp32, deterministic (no float atomics; fixed summation order that depends on (P, Q) only): two
 * calls give identical bits, map n's results are the same alone or inside a batch, and lobe l's results are the same alone
 * or among other lobes.
 * reni_lobe_convolve: for output directions o (out_dirs [P][3]), input directions d_i with weights w_i (in_dirs [Q][3],
 *   in_w [Q]), N maps (src, addressed as in reni_diffuse_convolve) and n_lobes lobes (1..16),
 *       t            = o . d_i                          (fp32: ox dx, then two fma, reni_diffuse_convolve's order)
 *       num[n,l,o,c] = sum_i f_l(t) w_i src(n, i, c)    den[l,o] = sum_i f_l(t) w_i
 *       out[n][l][o][c] = normalise ? (den > 0 ? num / den : 0) : scale num               out is [N][n_lobes][P][3]
 *   With m = clamp((1 + t) / 2, 0, 1) and tc = clamp(t, 0, 1), lobe l is kinds[l] with the one parameter params[l] (HOST
 *   arrays of n_lobes entries):
 *       RENI_LOBE_PHONG  f = tc^n                                 n > 0
 *       RENI_LOBE_BLINN  f = m^(s / 2)                            s > 0: (n . h)^s of the shader for view = normal
 *       RENI_LOBE_GGX    f = tc a^2 / (m (a^2 - 1) + 1)^2         1e-9 <= a <= 1, a = roughness^2: D(h) (n . l) of the split-sum
 *                                                                 prefilter under n = v = r, without 1 / pi
 *   A power is exp2(p log2(b)); b = 0 gives 0.  PHONG(1) and GGX(1) are the clamped cosine.  den is one more column of the
 *   same product (against ones), computed once per (lobe, o).  scale is ignored when normalising.
 *   ws: reni_lobe_workspace_bytes(N, P, Q, n_lobes) bytes, 256-byte aligned (always needed: the partial sums of the i split,
 *   which the library decides from (P, Q), and the division's operands).  n_lobes (3 N + 1) P and 3 Q < 2^30.
 * reni_envmap_lookup: out [N][P][3] = the bilinear sample, on the sphere, of map n's level at direction p.  src element
 *   (n, level, y, x, c) at src[n s[0] + level s[1] + y s[2] + x s[3] + c s[4]] (element strides >= 0, s[2] and s[3] < 2^31;
 *   Lv = 1 with s[1] = 0 reads plain maps).  Direction p of map n is dirs[n dirs_stride_n + 3 p + 0..2], dirs_stride_n 0
 *   (shared [P][3]) or 3 P (per map); it need not have unit length, and the zero vector samples the first row.  The
 *   coordinate chain is reni_rotate_envmap's from s on (phi = atan2f(sqrtf(s.x^2 + s.z^2), s.y), theta = atan2f(s.x, -s.z),
 *   the same row / col maps, clamps, pole and seam taps).  The level is level_const when level is NULL, else
 *   level[n level_stride_n + p] (level_stride_n 0 or P); it is clamped to [0, Lv - 1] and the result mixes floor(level) and
 *   the next level linearly, as one more lerp.  One launch, no workspace.  N, Lv <= 65535, H W < 2^30, W even, 3 N P < 2^30. */
#define RENI_LOBE_PHONG 0
#define RENI_LOBE_BLINN 1
#define RENI_LOBE_GGX 2
size_t reni_lobe_workspace_bytes(int64_t N, int64_t P, int64_t Q, int64_t n_lobes);
int reni_lobe_convolve(int64_t N, int64_t P, int64_t Q, const float* out_dirs, const float* in_dirs, const float* in_w,
                       const float* src, int64_t src_stride_n, int64_t src_stride_i, int64_t src_stride_c, int n_lobes,
                       const int32_t* kinds, const float* params, int normalise, float scale, float* out, void* ws,
                       size_t ws_bytes, void* stream);
int reni_envmap_lookup(int64_t N, int64_t Lv, int64_t H, int64_t W, int64_t P, const float* src, const int64_t src_strides[5],
                       const float* dirs, int64_t dirs_stride_n, const float* level, int64_t level_stride_n, float level_const,
                       float* out, void* stream);

/* ---- glossy lighting, backward: the transposes of the two operators above (reni_tu_glossy_bwd.hip; the autograd functions of
 * reni_amd/glossy.py).  Both operators are linear in the maps, so d loss / d map is their transpose applied to the upstream
 * gradient; directions, weights, levels and lobe parameters are constants.  fp32, deterministic (no float atomics, fixed
 * summation orders): two calls give identical bits and map n's gradient is the same alone or inside a batch.
 * reni_lobe_denominators: den[l][o] = sum_i f_l(o . d_i) w_i, [n_lobes][P] -- the denominators reni_lobe_convolve divides by
 *   when it normalises, bit for bit: the forward's own launch with no maps, only its column of ones (the split depends on
 *   (P, Q) only, and a column's sums do not depend on the columns beside it).  Equal to the unnormalised convolution, scale 1,
 *   of a map of ones.  ws: reni_lobe_denominators_workspace_bytes(P, Q, n_lobes) bytes, 256-byte aligned.
 * reni_lobe_convolve_backward: for grad_out [N][n_lobes][P][3], the upstream gradient of the forward's out,
 *       r[l][o]       = normalise ? (den[l][o] > 0 ? 1 / den[l][o] : 0) : scale
 *       dsrc(n, i, c) = w_i sum_l sum_o f_l(o . d_i) r[l][o] grad_out[n][l][o][c]
 *   written to grad_src[n grad_stride_n + i grad_stride_i + c grad_stride_c] (element strides >= 0; [N][Q][3] and planar
 *   [N][3][Q] both work; every element is written).  The same GEMM as the forward with rows and reduction swapped: t is built
 *   in the forward's fp32 order, the o range is split by the forward's rule with P and Q exchanged, the lobes of a kind are
 *   summed inside one launch, and the (kind, split) partial sums are added in that order.  den [n_lobes][P] (device, from
 *   the denominators entry above) is required iff normalise; scale is ignored when normalising.  The argument checks and
 *   error codes are the forward's.  ws: reni_lobe_backward_workspace_bytes(N, P, Q, n_lobes) bytes, 256-byte aligned.
 * reni_envmap_lookup_taps: for each direction the 8 texels the lookup reads -- 4 on floor(level), 4 on the next level, each
 *   as the element index level H W + y W + x of a contiguous [Lv][H][W] map -- and their effective weights
 *   {gr gc, gr fc, fr gc, fr fc} x {gl, fl} from the lookup's own coordinate chain (a copy of its four taps).  The next level weighs 0 unless
 *   fl > 0, as the forward reads it only then; a tap that is not used has weight 0 (and a valid index).  tap_index (int32) and
 *   tap_weight are [n_tables][P][8]; n_tables is 1 when directions and level are shared (both strides 0) and N otherwise.
 *   Lv H W < 2^31; the other limits are the lookup's.
 * reni_envmap_lookup_backward: grad_src [N][Lv][H][W][3] (contiguous, ALL of it written: 0 where nobody sampled) from
 *   grad_out [N][P][3], the tap weights, tap_order [n_tables][8 P] (int64: the taps' positions p 8 + k of a table in
 *   ascending order of their element index, ties in ascending position -- a stable sort) and offsets [n_tables][Lv H W + 1]
 *   (int64: element e owns tap_order[offsets[e] .. offsets[e + 1])).  One lane per (map, element) adds weight x upstream
 *   over its range in that order, for the three channels: a gather, no atomics.  n_tables = 1 serves all N maps.  A texel
 *   sampled by very many directions is summed by ONE lane: a known limit (a map's pole rows under a narrow field of view).
 *   An order entry outside [0, 8 P) is skipped and a range is clipped to the table, so a malformed table cannot become an
 *   address. */
size_t reni_lobe_denominators_workspace_bytes(int64_t P, int64_t Q, int64_t n_lobes);
int reni_lobe_denominators(int64_t P, int64_t Q, const float* out_dirs, const float* in_dirs, const float* in_w, int n_lobes,
                           const int32_t* kinds, const float* params, float* den, void* ws, size_t ws_bytes, void* stream);
size_t reni_lobe_backward_workspace_bytes(int64_t N, int64_t P, int64_t Q, int64_t n_lobes);
int reni_lobe_convolve_backward(int64_t N, int64_t P, int64_t Q, const float* out_dirs, const float* in_dirs, const float* in_w,
                                const float* grad_out, int n_lobes, const int32_t* kinds, const float* params, int normalise,
                                float scale, const float* den, float* grad_src, int64_t grad_stride_n, int64_t grad_stride_i,
                                int64_t grad_stride_c, void* ws, size_t ws_bytes, void* stream);
int reni_envmap_lookup_taps(int64_t n_tables, int64_t Lv, int64_t H, int64_t W, int64_t P, const float* dirs, int64_t dirs_stride_n,
                            const float* level, int64_t level_stride_n, float level_const, int32_t* tap_index, float* tap_weight,
                            void* stream);
int reni_envmap_lookup_backward(int64_t N, int64_t Lv, int64_t H, int64_t W, int64_t P, const float* grad_out, int64_t n_tables,
                                const float* tap_weight, const int64_t* tap_order, const int64_t* offsets, float* grad_src,
                                void* stream);

/* ---- split-sum microfacet shading from a prefiltered chain (reni_tu_splitsum.hip; reni_amd/glossy.py: sample, ggx_dfg,
 * shade_split_sum).  No reference counterpart.  fp32, deterministic (no float atomics, fixed summation orders).
 * reni_envmap_lookup_dquery: the derivative of the lookup's out with respect to its QUERY, contracted with grad_out [N][P][3].
 *   The arguments up to level_const are the lookup's, with its checks, limits and messages.  With (row, col) and the four
 *   folded taps b00 .. b11 of the lookup's own coordinate chain, fr, fc its fractions and gr = 1 - fr, gc = 1 - fc:
 *       d out / d row = gc (b10 - b00) + fc (b11 - b01)       d out / d col = gr (b01 - b00) + fr (b11 - b10)
 *   mixed over the two levels with the forward's weights; Gr = sum_c grad_out[c] d out[c] / d row, Gc likewise, and with
 *   rho^2 = q_x^2 + q_z^2 for the direction q (any length)
 *       d_dirs = row_scale Gr (q_y q_x / rho, -rho, q_y q_z / rho) / |q|^2 + col_scale Gc (-q_z, 0, q_x) / rho^2
 *   exactly 0 where the row clamp is active, where rho^2 = 0 (a pole direction) or |q|^2 = 0; never NaN or Inf for finite maps.
 *       d_level = [0 <= level <= Lv - 1] sum_c grad_out[c] (v(la + 1) - v(la))[c],  la = min(floor(level), Lv - 2)
 *   with v(l) the bilinear sample of level l: the slope of the piecewise-linear mix, right-sided at interior knots, left-sided
 *   at the top knot; 0 for Lv = 1, for a level outside the closed range and for a NaN level.
 *   d_dirs is [N][P][3] for per-map directions and [P][3], the sum over n ascending, for shared ones (dirs_stride_n = 0; Gr and
 *   Gc are summed, the chain rule applied once); d_level is [N][P] or, for a shared level array, [P].  Either may be NULL (that
 *   half is then not computed, and the other's bits do not change); both NULL is RENI_EINVAL, and so is d_level without a level
 *   array.  One launch, no workspace.
 * reni_ggx_dfg: out [2][R_r][R_v], the directional albedo of the microfacet material of reni_envmap_shade_ggx:
 *   out[0] = int k d omega, out[1] = int k f d omega over the hemisphere for N = (0, 0, 1), V = (sqrt(1 - x^2), 0, x),
 *   x = i / (R_v - 1), roughness r = r_min + j (1 - r_min) / (R_r - 1), alpha = r^2.  DEFINED as the midpoint rule on
 *   M_u x M_phi nodes u = (a + 1/2) / M_u, phi = 2 pi (b + 1/2) / M_phi of GGX's inverse-CDF parametrisation of the half vector,
 *   cos^2 theta_h = (1 - u) / (1 + (alpha^2 - 1) u), L = 2 (V.H) H - V, under which
 *       out[0] = int int 2 nl (V.H) / (nh (nl + lam(nl)) (nv + lam(nv))) [nl > 0][V.H > 0] du dphi,  lam(t) = sqrt(alpha^2 + (1 - alpha^2) t^2)
 *   and out[1] has the factor (1 - min(V.H, 1))^5 more.  2 <= R_v, R_r <= 1024, 1 <= M_u, M_phi <= 1024,
 *   R_v R_r M_u M_phi <= 2^28, 1e-3 <= r_min < 1.  One launch (a workgroup per entry), no workspace. */
int reni_envmap_lookup_dquery(int64_t N, int64_t Lv, int64_t H, int64_t W, int64_t P, const float* src,
                              const int64_t src_strides[5], const float* dirs, int64_t dirs_stride_n, const float* level,
                              int64_t level_stride_n, float level_const, const float* grad_out, float* d_dirs, float* d_level,
                              void* stream);
int reni_ggx_dfg(int64_t R_v, int64_t R_r, float r_min, int64_t M_u, int64_t M_phi, float* out, void* stream);

/* ---- UV-space textures: a material that lives on the surface (reni_tu_texture.hip; reni_amd/textures.py) --
 * A texture in the mesh's UV space is looked up per render pixel through the G-buffer, with a mip pyramid, and its gradient is
 * gathered back per texel.  No reference counterpart.  fp32, deterministic (no float atomics, fixed summation orders).
 * Mesh UVs: verts_uvs [Tn][2], faces_uvs [F][3] (int64, its own indexing); an entry outside [0, Tn) marks a face without UVs.
 * reni_mesh_pixel_uv: for pixel p of the S x S G-buffer with f = pix_to_face[p],
 *       uv[p]  = fmaf(b2, t2, fmaf(b1, t1, b0 t0)),  t_k = verts_uvs[faces_uvs[f][k]],  b = bary[p] (the rasteriser's own, NDC)
 *       jac[p] = (du/dcol, dv/dcol, du/drow, dv/drow) per pixel step: a constant of the face, from its NDC vertices with the
 *                rasteriser's chain (p R + T, / (z tan_half_fov), area edge(v2, v0, v1) + 1e-8, one pixel = -2 / S in NDC x and y)
 *   The pixel is INVALID when f is outside [0, F), a vertex or UV index of the face is out of range or uv is not finite: then
 *   uv = 0, jac = 0 and pix_valid[p] = -1 (else f).  pix_valid (int64 [S S]) may be NULL.  R [9], T [3] are host arrays.
 * The pyramid: level l is H_l x W_l = max(1, H0 >> l) x max(1, W0 >> l); L levels, 1 <= L <= 1 + log2(max(H0, W0)), L > 1 only
 *   for powers of two; stored back to back as [E][C], E = sum H_l W_l < 2^31, channels innermost, 1 <= C <= 8.
 * reni_texture_pyramid: fills levels 1 .. L - 1 from level 0, in place: texel (y, x) of level l + 1 is
 *   ((a(2y, 2x) + a(2y, 2x+1)) + (a(2y+1, 2x) + a(2y+1, 2x+1))) / 4 of level l, or (a0 + a1) / 2 of the two that exist where
 *   level l is one texel high or wide.  reni_texture_pyramid_backward: the transpose, in place on a gradient [E][C], from the
 *   coarsest level down: g_l(y, x) += r g_{l+1}(y >> 1, x >> 1), r = 1/4 or 1/2, for l = L - 2 .. 0; level 0 then holds
 *   d loss / d level 0 (the other levels hold partial sums and are of no further use).
 * reni_texture_taps: the 8 (element index into [E], weight) pairs of every pixel, tap_index int32 [P][8], tap_weight [P][8]:
 *       rho    = max(|(jac0 W0, jac1 H0)|, |(jac2 W0, jac3 H0)|) (hypotf: the squares neither overflow nor underflow),
 *                lambda = clamp(log2 rho + lod_bias, 0, L - 1); rho = 0 or not finite (a jac entry, or rho itself in fp32):
 *                lambda = 0; jac = NULL: lambda = clamp(lod_bias, 0, L - 1) for all pixels
 *       l0 = floor(lambda), fl = lambda - l0; the next level weighs 0 (and l1 = l0) when fl = 0 or l0 = L - 1
 *       RENI_TEX_CLAMP, align_corners 0:  x = clamp(u W_l - 1/2, 0, W_l - 1), y = clamp((1 - v) H_l - 1/2, 0, H_l - 1),
 *                x0 = floor x, x1 = min(x0 + 1, W_l - 1), fx = x - x0, likewise y      (grid_sample, border, at (2u - 1, 1 - 2v))
 *       RENI_TEX_REPEAT:  u' = u - floor u, x = u' W_l - 1/2, taps x0 = floor x and x0 + 1, both modulo W_l; y from 1 - v'
 *       align_corners 1 (L = 1 and RENI_TEX_CLAMP only):  x = clamp(u, 0, 1) (W0 - 1), y = (1 - clamp(v, 0, 1)) (H0 - 1)
 *       taps k = 0 .. 3 on l0: {gy gx, gy fx, fy gx, fy fx} (1 - fl) at (y0,x0) (y0,x1) (y1,x0) (y1,x1); k = 4 .. 7 on l1, x fl
 *   An unused tap has weight 0 and a valid index.  A pixel with pix_valid[p] < 0 (pix_valid may be NULL: none) or a uv that is not
 *   finite has all weights exactly 0 (index 0), so it fetches exactly 0.  uv [P][2] need not come from a mesh.
 * reni_texture_fetch: out[p][c] = sum_k w[p][k] tex[idx[p][k]][c], an fmaf chain over k = 0 .. 7 from 0; a tap of weight 0 is
 *   not read.  An index is clamped to [0, E): a table is trusted for weights, never for addresses.
 * reni_texture_fetch_backward: grad_tex [E][C] (ALL of it written: 0 where nobody sampled), grad_tex[e][c] = sum over the taps
 *   (p, k) with index e of w[p][k] grad_out[p][c], gathered through tap_order [8 P] (int64: the positions p 8 + k in ascending
 *   order of their element index, ties in ascending position -- a stable sort) and offsets [E + 1] (int64: element e owns
 *   tap_order[offsets[e] .. offsets[e + 1])).  A range of at most 128 entries is summed by one lane in that order.  A longer
 *   one is cut into chunks of 64 consecutive entries that the 64 lanes of a wave sum together -- lane j adds entry j of every
 *   chunk, in chunk order -- and the lane sums are combined by a fixed butterfly; the cut depends on offsets only, so two calls
 *   give identical bits, and a 1 x 1 top level costs 8 P / 64 steps per lane, not 8 P.  plain = 1: every range by one lane (kept
 *   for measurements).  An order entry outside [0, 8 P) is skipped and a range is clipped to the table: a malformed table cannot
 *   become an address.  Entries behind offsets[E] are never read: ops.texture_table sorts the taps of weight 0 there (every tap of
 *   an invalid pixel names element 0; left in the table they would make its range the longest).
 * Limits: P, S S < 2^28; V, F, Tn < 2^30; tap_index and tap_weight 16-byte aligned.  None of these launches is counted. */
#define RENI_TEX_CLAMP 0
#define RENI_TEX_REPEAT 1
int reni_mesh_pixel_uv(int64_t V, int64_t F, int64_t Tn, const float* verts, const int64_t* faces, const float* verts_uvs,
                       const int64_t* faces_uvs, const float* R, const float* T, float tan_half_fov, int64_t S,
                       const int64_t* pix_to_face, const float* bary, float* uv, float* jac, int64_t* pix_valid, void* stream);
int reni_texture_taps(int64_t P, const float* uv, const float* jac, const int64_t* pix_valid, int64_t L, int64_t H0, int64_t W0,
                      float lod_bias, int32_t wrap, int32_t align_corners, int32_t* tap_index, float* tap_weight, void* stream);
int reni_texture_pyramid(int64_t L, int64_t H0, int64_t W0, int64_t C, float* tex, void* stream);
int reni_texture_pyramid_backward(int64_t L, int64_t H0, int64_t W0, int64_t C, float* grad_tex, void* stream);
int reni_texture_fetch(int64_t P, int64_t E, int64_t C, const float* tex, const int32_t* tap_index, const float* tap_weight,
                       float* out, void* stream);
int reni_texture_fetch_backward(int64_t P, int64_t E, int64_t C, const float* grad_out, const float* tap_weight,
                                const int64_t* tap_order, const int64_t* offsets, int32_t plain, float* grad_tex, void* stream);

/* ---- HDR image epilogue / prologue ------------------------------------------------
 * reni_unnormalise_srgb replaces, on the device and in one call, the reference's viewing chain
 *   UnMinMaxNormlise(minmax)   src/utils/custom_transforms.py:14-21   y = exp(0.5 (x + 1)(m1 - m0) + m0)
 *   sRGB                       src/utils/utils.py:30-42               y / q_b, clamp to [0,1], sRGB transfer curve, where
 *                              q_b = the nested 0.98-quantile over channels, then rows, then columns of image b
 *                              (torch.quantile semantics: rank q (n - 1) in fp32, ATen's lerp between the neighbours)
 * as the image callbacks apply it to a model output (src/lightning/callbacks.py; RENI_module.py:108 un-normalises in the
 * FIT_INVERSE step).
 *   img        : element (b, c, h, w) at img[b*strides[0] + c*strides[1] + h*strides[2] + w*strides[3]] (floats) -- a
 *                model output [B, H*W, 3] is read in place with strides {3HW, 1, 3W, 3}, a [B,3,H,W] batch with {3HW, HW, W, 1}
 *   unnormalise: 1 = apply UnMinMaxNormlise(minmax0, minmax1) first, 0 = img is linear already (plain sRGB())
 *   srgb       : 1 = produce out_srgb [B][3][H][W]; 0 = only the linear image
 *   out_linear : [B][3][H][W] linear HDR, or NULL when not wanted (then srgb must be 1)
 *   ws         : reni_image_workspace_bytes(B, H, W) bytes, 256-byte aligned (needed when srgb = 1); H, W <= 4096
 *   NaN propagates as in torch: a NaN (or an infinite largest channel) in an image makes its exposure, and so its whole sRGB
 *   image, NaN, and no other image's; an exposure of 0 gives 1 for lit pixels and NaN (0 / 0) for zero ones.
 * reni_minmax_normalise is the forward transform MinMaxNormalise (custom_transforms.py:4-12) over the n elements of one
 * image: clip to [smallest positive, largest finite value of the image] -> log -> 2 (. - m0) / (m1 - m0) - 1.  A NaN enters
 * neither bound and stays NaN; -0.0 is a zero, not a bound. */
size_t reni_image_workspace_bytes(int64_t B, int64_t H, int64_t W);
int reni_unnormalise_srgb(int64_t B, int64_t H, int64_t W, const float* img, const int64_t strides[4], int32_t unnormalise,
                          double minmax0, double minmax1, int32_t srgb, float* out_srgb, float* out_linear, void* ws,
                          size_t ws_bytes, void* stream);
int reni_minmax_normalise(int64_t n, const float* img, double minmax0, double minmax1, float* out, void* ws, size_t ws_bytes,
                          void* stream);
/* reni_minmax_normalise_batch: the same transform over N images of n contiguous elements each ([N][n]); the clip bounds are
 * each image's own, every element goes through the expression reni_minmax_normalise uses (image b's result is bit-identical
 * to a single-image call), and with nan_to_num != 0 torch.nan_to_num follows (NaN -> 0, +-inf -> +-FLT_MAX; datasets.py:72).
 * ws: reni_minmax_batch_workspace_bytes(N) bytes, 256-byte aligned.  1 <= N <= 65535, 1 <= n < 2^30. */
size_t reni_minmax_batch_workspace_bytes(int64_t N);
int reni_minmax_normalise_batch(int64_t N, int64_t n, const float* imgs, double minmax0, double minmax1, int32_t nan_to_num,
                                float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- image resampling and blur (reni_tu_resample.hip; the resident dataset, baselines.resizeImage / blurIBL) -------------
 * fp32, no atomics: two calls give identical bits and an image's result is the same alone or inside a batch.
 * reni_resample: the separable table-driven gather
 *     out[n][c][y][x] = sum_(j < row_taps) row_w[y][j] ( sum_(k < col_taps) col_w[x][k] src(n, c, row_idx[y][j], col_idx[x][k]) )
 *   with src(n, c, y, x) = src[n s0 + c s1 + y s2 + x s3] (element strides >= 0: channel-last [H][W][3] is {0, 1, 3 W, 3},
 *   planar [N][3][H][W] is {3HW, HW, W, 1}) and out planar [N][C][Hd][Wd].  The tables are device arrays built by the host
 *   (reni_amd/resample.py: coordinates in exact integers / float64, rounded to fp32 once): row_idx, row_w [Hd][row_taps],
 *   col_idx, col_w [Wd][col_taps], 1 <= taps <= 8.  The interpolation mode lives in the tables alone.  Indices are clamped to
 *   the source on the device, so a bad table cannot read outside it.  N, C <= 65535, Hs Ws < 2^30, N C Hd Wd < 2^30.
 * reni_gaussian_blur: scipy.ndimage.gaussian_filter(img2d, sigma) per channel (blurIBL, spherical_harmonics.py:564-569):
 *   separable, axis 0 (rows) first, then axis 1; boundary `reflect` (d c b a | a b c d | d c b a); the fp32 intermediate lives
 *   in ws.  weights: device array [2 radius + 1] (the host normalises exp(-x^2 / 2 sigma^2) in float64, radius =
 *   int(4 sigma + 0.5)).  Element (c, y, x) of src and of out at c s0 + y s1 + x s2 (out has the input's layout).
 *   ws: reni_blur_workspace_bytes(C, H, W) bytes, 256-byte aligned. */
int reni_resample(int64_t N, int64_t C, int64_t Hs, int64_t Ws, int64_t Hd, int64_t Wd, const float* src,
                  const int64_t src_strides[4], const int32_t* row_idx, const float* row_w, int32_t row_taps,
                  const int32_t* col_idx, const float* col_w, int32_t col_taps, float* out, void* stream);
size_t reni_blur_workspace_bytes(int64_t C, int64_t H, int64_t W);
int reni_gaussian_blur(int64_t C, int64_t H, int64_t W, const float* src, const int64_t strides[3], const float* weights,
                       int32_t radius, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- rotation of equirectangular environment maps (reni_tu_rotate.hip; reni_amd/rotation.py, ResidentDataset's augmentation) --
 * No reference counterpart (the reference rotates latents, never images).  out[b] is source image b turned by R_b:
 *     out[b](d) = src[b](R_b^T d)        so that, for an equivariant model f,  f(Z R^T, D) = rotate(f(Z, D), R).
 * Grid: H rows, W columns, W even; pixel (r, c) has phi = pi (r + 1/2) / H, theta = pi ((c + 1/2) / (W / 2) - 1) and direction
 * d = (sin phi sin theta, cos phi, -sin phi cos theta) (utils.get_directions when W = 2 H).  For output pixel (r, c):
 *     s = R^T d,  phi_s = atan2(sqrt(s.x^2 + s.z^2), s.y),  theta_s = atan2(s.x, -s.z),
 *     row = phi_s / pi H - 1/2,  col = (theta_s / pi + 1) W / 2 - 1/2.
 * Sampling is on the sphere: tap (i, j) with i < 0 is row -1 - i, column j + W / 2; with i >= H row 2 H - 1 - i, column j + W / 2
 * (the row beyond a pole is the same row seen from the other side); then the column modulo W.  RENI_ROTATE_BILINEAR: the four
 * taps floor(row), floor(row) + 1 x floor(col), floor(col) + 1 with the usual weights; RENI_ROTATE_NEAREST: the tap at
 * floor(row + 1/2), floor(col + 1/2) (masks).  fp32, one launch on `stream`, no atomics, no workspace, no host synchronisation:
 * two calls give identical bits, and an image's result is the same alone, inside a batch and through src_index.
 *   src, src_strides: as reni_resample (planar, channel-last, or a model output [B][P][3] = {3 H W, 1, 3 W, 3} read in place)
 *   src_index: NULL (image b is source b) or a device array [B]: image b is source src_index[b] of n_src, clamped to
 *              [0, n_src) on the device -- the gather of a batch out of a level tensor, in the same launch
 *   rot, rot_stride: device array [B][9], row-major R per image (stride 9), or one shared R (stride 0).  Not checked for
 *              orthogonality here (reni_amd/rotation.py does); s is used as it comes, atan2 needs no unit length
 *   row_trig [H][2] = (sin phi, cos phi), col_trig [W][2] = (sin theta, cos theta) of the grid above: device arrays the host
 *              builds in float64 and rounds to fp32 once.  sqrt and the two atan2f of a pixel run on the device: with a fresh
 *              rotation per image and step, host tables of the SOURCE coordinates would be the bottleneck.
 *   out: planar [B][C][H][W].  B, C <= 65535, H W < 2^30, src_strides[2] and [3] < 2^31. */
#define RENI_ROTATE_NEAREST 0
#define RENI_ROTATE_BILINEAR 1
int reni_rotate_envmap(int64_t B, int64_t C, int64_t H, int64_t W, const float* src, const int64_t src_strides[4],
                       const int64_t* src_index, int64_t n_src, const float* rot, int64_t rot_stride, const float* row_trig,
                       const float* col_trig, int32_t mode, float* out, void* stream);

/* ---- scores of environment-map pairs (reni_tu_metrics.hip; reni_amd/metrics.py) ------------------------------------------------
 * No reference counterpart (the reference's evaluation composes these from tensor operations).  A prediction and a target, B images
 * of 3 x H x W each, are read in place: element (b, c, h, w) of an image at ptr[b s[0] + c s[1] + h s[2] + w s[3]] (element strides
 * >= 0, as reni_resample and reni_unnormalise_srgb take them: planar [B][3][H][W] is {3HW, HW, W, 1}, a model output [B][P][3] is
 * {3HW, 1, 3W, 3}).  weight: element (b, h, w) at weight[b s[0] + h s[1] + w s[2]], any stride may be 0 (sin phi per row is an [H]
 * array with {0, 1, 0}, a shared mask {0, W, 1}); NULL is weight 1.  Weights are expected >= 0; a pixel of weight 0 is not there.
 * space: what is compared, mapped in registers (nothing mapped is written to memory), prediction and target alike:
 *     RENI_SPACE_STORED   the numbers as given
 *     RENI_SPACE_LINEAR   exp(0.5 (x + 1)(minmax1 - minmax0) + minmax0), UnMinMaxNormlise: the expression of reni_unnormalise_srgb
 *     RENI_SPACE_SRGB     linear / exposure[b], clamped to [0, 1], the sRGB transfer curve (utils.sRGB's, reni_unnormalise_srgb's).
 *                         exposure: device array [B] from the caller (metrics.exposure: the nested 0.98-quantile of the linear
 *                         target), applied to BOTH images: a pair is judged under one exposure.
 * minmax0 / minmax1 are read in the mapped spaces only (minmax1 > minmax0), exposure in RENI_SPACE_SRGB only.
 * fp32 on the device, no float atomics, sums in an order that depends on (H, W) only, no host synchronisation, launches on `stream`
 * only: two calls give identical bits; image b scores the same alone and inside a batch, planar and as a model output.
 * ws (both calls): reni_pair_stats_workspace_bytes(B, H, W) bytes, 256-byte aligned.  1 <= B <= 65535, H W < 2^30.
 *
 * reni_pair_stats: one pass, every pixel read once; out[B][8], over pixels i (weight w_i) and channels c of mapped p, t:
 *     [0] sum_i w_i                        [4] max of t over the pixels with w_i > 0   (-inf when there is none)
 *     [1] sum_i w_i sum_c (p - t)^2        [5] min of t over the pixels with w_i > 0   (+inf when there is none)
 *     [2] sum_i w_i sum_c |p - t|          [6] sum_i w_i sum_c t^2
 *     [3] sum_i w_i cos(p_i, t_i)          [7] sum_i w_i sum_c t
 *   cos is the RGB-vector cosine of F.cosine_similarity(dim = channel, eps = 1e-20).  Workgroups write fp32 partials to ws; a second
 *   kernel adds an image's partials in double in a fixed order and rounds once.  A pixel of weight 0 is skipped, not multiplied by 0:
 *   a NaN, an infinity or an overflowing exponential there changes no bit of any entry.  With no pixel of weight > 0 the six sums
 *   are exactly 0, [4] is -inf and [5] is +inf.
 *
 * reni_ssim: the mean SSIM of Wang et al. 2004 per image, out[B]: an 11 x 11 Gaussian window, sigma 1.5, normalised (the host builds
 *   the 11 weights in float64 and rounds them once), C1 = (0.01 L)^2, C2 = (0.03 L)^2, per channel of the mapped images
 *       ssim = (2 mu_p mu_t + C1)(2 cov + C2) / ((mu_p^2 + mu_t^2 + C1)(var_p + var_t + C2)),
 *   mu, var, cov from the five windowed moments E[p], E[t], E[p^2], E[t^2], E[p t]; the three channels are averaged.
 *     RENI_SSIM_SPHERE  every pixel has a window; its taps are taken on the sphere by the rule of reni_rotate_envmap: row i < 0 is
 *                       row -1 - i at column j + W / 2, row i >= H is row 2 H - 1 - i at column j + W / 2, then the column modulo W.
 *                       W even, H >= 5.  out[b] = sum_i w_i ssim_i / sum_i w_i.
 *     RENI_SSIM_PLANAR  the published image definition: only the windows that lie inside the image, an (H - 10) x (W - 10) map,
 *                       unweighted mean.  weight must be NULL; H, W >= 11.
 *   map_out: NULL, or [B][H][W]: the channel-mean SSIM of every pixel (planar mode: zero on the border of 5).
 *   A weight acts on the MEAN only; a window has no per-tap weight.  A pixel of weight 0 is left out of out[b], but its value is a
 *   tap of the 11 x 11 window of every pixel around it (on the sphere by the tap rule above, across a pole and around the seam).
 *   If that value is not finite once mapped (a NaN; an infinity in RENI_SPACE_STORED; +inf or an overflowing exponential in
 *   RENI_SPACE_LINEAR -- exp(-inf) is 0, and the clamp of RENI_SPACE_SRGB turns an infinite radiance into 1), map_out is NaN on
 *   exactly the pixels whose window holds it and unchanged everywhere else, and out[b] is unchanged once every pixel of that set has
 *   weight 0; otherwise out[b] is NaN.  With no pixel of weight > 0, out[b] is 0 / 0 = NaN.
 *   One kernel holds a 32 x 32 tile plus halo of both mapped images in LDS and forms the moments separably; the values go straight
 *   into the workgroup's partial sum, no moment image is written to memory. */
#define RENI_SPACE_STORED 0
#define RENI_SPACE_LINEAR 1
#define RENI_SPACE_SRGB 2
#define RENI_SSIM_SPHERE 0
#define RENI_SSIM_PLANAR 1
size_t reni_pair_stats_workspace_bytes(int64_t B, int64_t H, int64_t W);
int reni_pair_stats(int64_t B, int64_t H, int64_t W, const float* pred, const int64_t pred_strides[4], const float* target,
                    const int64_t target_strides[4], const float* weight, const int64_t weight_strides[3], int32_t space,
                    double minmax0, double minmax1, const float* exposure, float* out, void* ws, size_t ws_bytes, void* stream);
int reni_ssim(int64_t B, int64_t H, int64_t W, const float* pred, const int64_t pred_strides[4], const float* target,
              const int64_t target_strides[4], const float* weight, const int64_t weight_strides[3], int32_t space,
              double minmax0, double minmax1, const float* exposure, float L, int32_t mode, float* out, float* map_out, void* ws,
              size_t ws_bytes, void* stream);

/* ---- environment maps as importance-sampled light lists (reni_tu_lights.hip; reni_amd/lighting.py) ----------------------------
 * No reference counterpart (the reference sums every texel of a map wherever it lights something).  B maps of 3 x H x W on RENI's
 * grid (W even, H = W / 2, W <= 4096, 1 <= B <= 65535) are read in place through four element strides as reni_pair_stats reads
 * them; space is RENI_SPACE_STORED (the numbers are radiance already) or RENI_SPACE_LINEAR (the expression of reni_unnormalise_srgb,
 * in registers); RENI_SPACE_SRGB is RENI_EINVAL.  solid_angle [H] is the per-texel solid angle omega_i of row i, row_cos [H + 1]
 * (double) is cos(i pi / H), dirs_table [H W][3] the texel-centre directions: host tables, so the library holds no grid convention.
 * fp32 storage, no float atomics, no host synchronisation, launches on `stream` only; every sum runs in an order that depends on
 * (H, W) or S only: two calls give identical bits, and image b's results are the same alone and inside a batch.
 *
 * reni_light_table_build: the sampling distribution.  Per texel f = max(0, 0.2126 r + 0.7152 g + 0.0722 b) omega_i mask, formed in
 *   double and rounded to fp32 once (a NaN counts as 0); F_b = sum f.  mask: element (b, h, w) at mask[b s[0] + h s[1] + w s[2]], any
 *   stride may be 0, NULL is 1, expected >= 0.  With eps = uniform_mix in [0, 1]
 *       pmf  [B][H][W] = (1 - eps) f / F_b + eps omega_i / sum_i (W omega_i)      (F_b zero or not finite: eps = 1 for that image)
 *       cond [B][H][W] = inclusive prefix sum of the row's pmf / the row's sum    (a row without mass: (j + 1) / W)
 *       marg [B][H]    = inclusive prefix sum of the row sums / their total
 *   Everything behind f is double arithmetic on the rounded f, rounded to fp32 once.  The prefix sums come from a parallel scan (a
 *   fixed order, not the sequential one); each is divided by the scan's own value at the last entry with mass, and a running
 *   maximum behind the division makes every CDF ascending, exactly flat over an entry whose pmf is 0, and exactly 1.0f from the
 *   last entry with mass on.  ws: reni_light_table_workspace_bytes(B, H, W) bytes, 256-byte aligned.
 *
 * reni_light_sample: S lights per map by inverse-CDF sampling.  u: uniforms in [0, 1) (not checked), sample k of image b at
 *   u[b u_stride_b + 2 k] (u_stride_b 0: one [S][2] set for all images; 2 S: [B][S][2]).  Row i = the number of entries of marg[b]
 *   that are <= u0, at most H - 1; column j = the number of entries of cond[b][i] that are <= u1, at most W - 1 (numpy's
 *   searchsorted(side = "right"): a texel without mass is never chosen).  Per sample, with t = i W + j:
 *       index    [B][S]    = t                      pdf      [B][S]    = pmf[t] / omega_i   (per steradian)
 *       radiance [B][S][3] = the mapped texel       colors   [B][S][3] = radiance texel_weight[t] / (S pmf[t])   (texel_weight NULL: 1)
 *       dirs     [B][S][3] = dirs_table[t] (jitter 0), or (jitter 1) uniform in solid angle inside the texel: with t_r, t_c where u0,
 *                            u1 lie between the CDF entries around i, j:  cos phi = row_cos[i] - t_r (row_cos[i] - row_cos[i + 1]),
 *                            theta = 2 pi (j + t_c) / W - pi,  d = (sin phi sin theta, cos phi, -sin phi cos theta)   (in double)
 *   so that sum_s colors_s g(dirs_s) estimates sum_t texel_weight_t L_t g(d_t).
 *
 * reni_lights_irradiance: out [B][P][3] = scale sum_s max(0, n_p . dirs_bs) colors_bs for normals [P][3] (normals_stride_b 0) or
 *   [B][P][3] (3 P) and light lists dirs, colors [B][S][3]; lights are staged in LDS and added in ascending s, one fmaf chain per
 *   output channel.  1 <= B <= 65535, B P < 2^28 and B S < 2^28 (reni_light_sample: B S < 2^28 as well). */
size_t reni_light_table_workspace_bytes(int64_t B, int64_t H, int64_t W);
int reni_light_table_build(int64_t B, int64_t H, int64_t W, const float* img, const int64_t img_strides[4], const float* mask,
                           const int64_t mask_strides[3], int32_t space, double minmax0, double minmax1, const float* solid_angle,
                           double uniform_mix, float* pmf, float* cond, float* marg, void* ws, size_t ws_bytes, void* stream);
int reni_light_sample(int64_t B, int64_t H, int64_t W, int64_t S, const float* pmf, const float* cond, const float* marg,
                      const float* img, const int64_t img_strides[4], int32_t space, double minmax0, double minmax1,
                      const float* u, int64_t u_stride_b, const float* dirs_table, const float* solid_angle,
                      const double* row_cos, const float* texel_weight, int32_t jitter, int32_t* index, float* dirs, float* pdf,
                      float* radiance, float* colors, void* stream);
int reni_lights_irradiance(int64_t B, int64_t P, int64_t S, const float* normals, int64_t normals_stride_b, const float* dirs,
                           const float* colors, float scale, float* out, void* stream);

/* ---- the data-parallel exchange step over RCCL -------------------------------
 * Replaces, for the flat decoder gradient, what Lightning's DDP wrapper does in the reference (run.py:97-110:
 * strategy="ddp" -> NCCL all-reduce of every parameter's gradient, mean over ranks): ONE in-place ncclAllReduce(sum) of
 * the n floats at `flat`, then flat *= scale (1 / world_size for DDP's mean), both on `stream`.  Latent rows are owned by
 * one rank each and are never exchanged.
 * `comm` is an ncclComm_t.  It may come from any RCCL in the process; the three helpers below make one without PyTorch:
 * rank 0 calls reni_rccl_unique_id and hands the 128 bytes to the other ranks (any side channel), then every rank calls
 * reni_rccl_comm_create (collective) with its device current.  librccl is loaded on first use: without it these four
 * return RENI_EUNSUPPORTED and the rest of the library is unaffected. */
typedef struct { char internal[128]; } reni_rccl_id; /* layout of ncclUniqueId */
int reni_rccl_unique_id(reni_rccl_id* id);
int reni_rccl_comm_create(const reni_rccl_id* id, int32_t nranks, int32_t rank, void** comm);
int reni_rccl_comm_destroy(void* comm);
int reni_allreduce_grads(void* comm, float* flat, size_t n, float scale, void* stream);

/* Launch geometry chosen for (B,P): workgroups, threads, dynamic LDS bytes (diagnostics). */
int reni_launch_info(const reni_plan* plan, int64_t B, int64_t P, int32_t* info4);

/* Which kernels a backward call of this shape will take (diagnostics; no reference counterpart -- the reference has one path).
 * info8 = { persistent kernels (k_reni_train_bf16) 0/1, dW_1 kernel 0 none / 1 k_reni_dw1_ring / 2 k_reni_dw1 /
 *           3 k_reni_l0_ring behind the L0X training instance (then, and only then, the training kernel's weight-gradient partials of
 *           layers >= 2 are in the quad-row layout and are summed by the quad-row reducer: DESIGN.md 4.2e, 4.3),
 *           side stream 0/1 (1: a side stream is ALLOWED for this plan -- a call then forks onto it only if it is not an L0X call and,
 *           for a concat decoder, has at least eight tiles per workgroup), images per chunk of the H = 256 training path (= B: one pass), operand stream 0/1,
 *           fragment stream 0 / 1 bf16 / 2 fp32, environment overrides in force (bit 0 RENI_NO_PERSIST, 1 RENI_NO_SIDE_STREAM,
 *           2 RENI_FRAG_WS_CAP_MB, 3 RENI_DW1_OLD, 4 RENI_NO_L0X, 5 RENI_TRAIN_WG = n: at most n workgroups for the persistent
 *           training instances; 0 in a clean environment), workgroups }.
 * The selectors are read from the environment ONCE, at reni_plan_create (a switch is on when its variable is set to anything but ""
 * or "0"); every alternative is a tested, correct path, and
 * bench.py prints this record so that a stray variable cannot silently change what is measured. */
int reni_path_info(const reni_plan* plan, int64_t B, int64_t P, uint32_t flags, int32_t* info8);

/* Data-parallel overlap hook (reference: DDP overlaps its bucketed all-reduce with the tail of backward, run.py:97).  While an
 * event is set (thread-local; NULL clears it), every reni_forward_loss_backward[_rows] call with RENI_NEED_DW records it on the
 * call's stream at the point where dparams[n_first + H*H + H ...) -- layers >= 2 and the head, 28 % of the gradient at config 2 -- is
 * final: on the persistent path that is before k_reni_dw1 runs (~0.13 ms before the call's work ends), on every other path at
 * the end of the call.  The caller makes its communication stream wait for the event and all-reduces that slice there, the
 * rest behind the call as before.  `hip_event` is a hipEvent_t created by the caller on the buffers' device. */
int reni_set_grad_ready_event(void* hip_event);

/* Kernel launches counted so far in this process, on all streams; reset != 0 returns the count and sets it to zero.  Counted:
 * every launch of the model's entry points (forward, backward, training and latent steps, optimisers, weight lists), of the
 * image, metrics, lights and visibility entry points, and of reni_lobe_denominators, reni_lobe_convolve_backward,
 * reni_envmap_lookup_taps and reni_envmap_lookup_backward.  NOT counted: the shader, raster, baseline (SG, SH), diffuse,
 * resample, blur, rotate and texture entry points, reni_lobe_convolve and reni_envmap_lookup.
 * bench.py reports launches per step: at small problems a step costs its dependent launches. */
int64_t reni_launch_count(int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* RENI_HIP_H */

/* libtacorl_hip.so - C ABI of the MI355X (gfx950) TACO-RL offline-training hot path.
 *
 * The reference (ErickRosete/tacorl) is pure Python and has no FFI for this path
 * (SURVEY.md section 8b): every entry point below replaces a stock-torch op sequence
 * inside the reference module named in its comment.  Contract for ALL functions:
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors);
 *     the caller keeps it alive until `stream` has been synchronised;
 *   - work is enqueued asynchronously on `stream`; nothing allocates, nothing
 *     synchronises (hipGraph-capturable); scratch comes from the caller through
 *     (ws, ws_bytes) and is sized by the matching *_ws_bytes query;
 *   - return 0 on success, negative errno-style code otherwise (never throws);
 *     tacorl_hip_last_error() gives the text for the calling thread;
 *   - "problem batches": arrays of `nprob` pointers describe independent problems of
 *     the same geometry (actor / q1 / q2 / target nets) that run in ONE launch.
 *   - fp32 row-major tensors; images NHWC; conv weights [CO][KH][KW][CI].
 */
#ifndef TACORL_HIP_H
#define TACORL_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* tacorl_stream_t; /* hipStream_t */

#define TACORL_MAXP 16 /* max problems per batched call */
enum { TACORL_F32 = 0, TACORL_BF16 = 1 };               /* storage / MFMA operand dtype */
enum { TACORL_ACT_NONE = 0, TACORL_ACT_RELU = 1, TACORL_ACT_SILU = 2, TACORL_ACT_TANH = 3 };
/* TANH (goal encoders with last_layer_activation: Tanh): taken by tacorl_mlp_fwd / tacorl_mlp_bwd and the fused
 * tacorl_mlp_fwd_fused* / tacorl_mlp_bwd_fused_* entry points, as a hidden or as the LAST activation; its derivative is
 * taken from the saved output (1 - y^2).  A LAST-layer TANH is a pass d_out * (1 - y^2) in front of the usual chain;
 * tacorl_mlp_bwd_fused_dgrad leaves its result in the workspace, where tacorl_mlp_bwd_fused_wgrad (same workspace, called
 * after it, as for the hidden layers' dZ) reads it.  The many-row and persistent MLP kernels are SiLU-only and are not
 * selected. */

int tacorl_hip_version(void);
int tacorl_hip_init(int device);             /* idempotent; checks the device is gfx950 */
const char* tacorl_hip_last_error(void);
/* tracing aid: marks[slot] = device wall clock (100 MHz ticks) when the stream reaches this point */
int tacorl_time_mark(unsigned long long* marks, int slot, tacorl_stream_t stream);
/* calibration aid: a 1-thread kernel that runs for `ticks` of that clock and stores its own begin / end in marks[slot],
 * marks[slot + 1] - an event bracket around it minus that difference is the bracket's overhead for a kernel of that length */
int tacorl_time_spin(unsigned long long* marks, int slot, long ticks, tacorl_stream_t stream);

/* ---- primitives ------------------------------------------------------------------ */
/* y = act(x W^T + b), optional pre-activation z.  Replaces nn.Linear (+F.silu / nn.ReLU):
 * reference networks/actor_critic/actor.py:252-270, critic.py:92-97, goal_encoder.py:17-23. */
int tacorl_linear_fwd(int nprob, const float* const* x, int ldx, const float* const* w,
                      const float* const* b, float* const* y, float* const* z, const int* M,
                      int K, int N, int act, int compute_dtype, tacorl_stream_t stream);
/* y = act(x W^T + b + addend), y with leading dim ldy: one ReLU-RNN time step
 * (torch nn.RNN relu; reference networks/action_decoders/rnn_models.py:5-16). */
size_t tacorl_linear_add_fwd_ws_bytes(int nprob, const int* M, int K, int N);
/* ws (may be NULL): scratch for the split-reduction path used when M is too small to fill the chip. */
int tacorl_linear_add_fwd(int nprob, const float* const* x, int ldx, const float* const* w,
                          const float* const* b, const float* const* addend, int ld_add, float* const* y,
                          int ldy, const int* M, int K, int N, int act, int compute_dtype, void* ws,
                          size_t ws_bytes, tacorl_stream_t stream);
/* y = act(x W^T + b + addend) with bf16 operands resident in HBM (x [M][K], W [N][K]; K % 128 == 0,
 * N % 32 == 0): the stacked ReLU-RNN of the action decoder (reference rnn_models.py:5-16, torch nn.RNN) -
 * recurrent step (M = batch) and per-layer input projection (M = batch*T).  One launch, no split-K: a
 * 4-stage LDS-DMA ring streams K.  Writes y fp32 and, if y_bf16 != NULL, the bf16 copy that is the next
 * step's operand.  bf16 MFMA, fp32 accumulate. */
int tacorl_rnn_linear_supported(int M, int K, int N);
int tacorl_rnn_linear_fwd(const void* x_bf16, const void* w_bf16, const float* bias, const float* addend,
                          int ld_add, float* y, void* y_bf16, int M, int K, int N, int act,
                          tacorl_stream_t stream);
/* nprob <= 4 independent y = act(x W^T + b + addend) of one shape (M, K, N) in one launch, one activation per
 * problem: the wavefront schedule of the stacked RNN (launch s = recurrent step s-2l of every layer l plus
 * the input projection of step s-2l+1 of layers l >= 1).
 * In this entry and its _twin / _ext forms:
 *   x_bf16[p] == NULL: a zero operand (the RNN's first step, h_{-1} = 0) - its K tiles are neither fetched nor multiplied;
 *     bit-identical to passing a buffer of zeros for finite weights.  Only for a problem without twin rows (with twin rows:
 *     TACORL_EINVAL); without a K extension either, the result is act(b + addend).
 *   y[p] == NULL: the fp32 result is not stored, only the bf16 copy (which must then be given). */
int tacorl_rnn_linear_fwd_batch(int nprob, const void* const* x_bf16, const void* const* w_bf16,
                                const float* const* bias, const float* const* addend, int ld_add,
                                float* const* y, void* const* y_bf16, int M, int K, int N, const int* acts,
                                tacorl_stream_t stream);
/* tacorl_rnn_linear_fwd_batch with twin rows: problem p additionally computes y2[p] = act(x2[p] W[p]^T + b[p] + addend2[p])
 * for M2 more rows held in other buffers - the same weights, read once (every problem of the launch carries twin rows).
 * PlayLMP.training_step: the logging-only random-plan pass of the action decoder (reference play_lmp_for_rl.py:243-252)
 * rides in the launches of the real pass. */
int tacorl_rnn_linear_fwd_batch_twin(int nprob, const void* const* x_bf16, const void* const* x2_bf16,
                                     const void* const* w_bf16, const float* const* bias, const float* const* addend,
                                     const float* const* addend2, int ld_add, float* const* y, float* const* y2,
                                     void* const* y_bf16, void* const* y2_bf16, int M, int M2, int K, int N,
                                     const int* acts, tacorl_stream_t stream);
/* The same launch with an optional K extension per problem (x_ext[p] != NULL; NULL arrays / entries: none):
 * y[p] = act(x[p] W[p]^T + x_ext[p] w_ext[p]^T + b[p] + bias2[p] + addend[p]), x_ext bf16 [M][128] (x2_ext [M2][128] for the twin
 * rows), w_ext bf16 [N][128], zero padded beyond the real width.  Layer 0's cell of the action decoder's ReLU-RNN as ONE
 * contraction over [h_{t-1} | x_t] - reference networks/action_decoders/rnn_models.py:5-16 (torch nn.RNN: h_t = relu(W_ih x_t +
 * b_ih + W_hh h_{t-1} + b_hh)) - instead of a separate input-projection launch + fp32 addend.  M2 = 0: no twin rows. */
int tacorl_rnn_linear_fwd_batch_ext(int nprob, const void* const* x_bf16, const void* const* x2_bf16,
                                    const void* const* w_bf16, const float* const* bias, const float* const* addend,
                                    const float* const* addend2, int ld_add, float* const* y, float* const* y2,
                                    void* const* y_bf16, void* const* y2_bf16, int M, int M2, int K, int N,
                                    const int* acts, const void* const* x_ext, const void* const* x2_ext,
                                    const void* const* w_ext, const float* const* bias2, tacorl_stream_t stream);
/* The ring GEMM with row strides, for the bidirectional ReLU-RNN plan recognition (reference
 * plan_encoders/plan_recognition_tanh_net.py: nn.RNN(num_layers=2, bidirectional=True)): nprob <= 4 problems
 * y[p] = act(x[p] W[p]^T + x_ext[p] w_ext[p]^T + bias[p] + bias2[p] + addend[p]) * [mask_src[p] > 0] of one shape (M, K, N),
 * x rows ldx apart (ldx % 8 == 0), y / y_bf16 / mask_src rows ldy apart (ldy % 4 == 0): both directions' step of a layer in
 * one launch over column slices of the interleaved [T][B][2H] state; BPTT steps with W^T as w and the saved state as mask_src.
 * Any array entry but x / w / y may be NULL; x_ext [M][128], w_ext [N][128] bf16 as in tacorl_rnn_linear_fwd_batch_ext. */
int tacorl_rnn_linear_ld_supported(int M, int K, int N, int ldx, int ldy);
int tacorl_rnn_linear_ld(int nprob, const void* const* x_bf16, int ldx, const void* const* w_bf16, const float* const* bias,
                         const float* const* bias2, const float* const* addend, int ld_add, const void* const* x_ext,
                         const void* const* w_ext, const float* const* mask_src, float* const* y, void* const* y_bf16, int ldy,
                         int M, int K, int N, int act, tacorl_stream_t stream);
/* out_bf16[(t*B + b)][0..127] = bf16([plan[b] (P) | emb[(b*T + t)] (E) | zeros]) for t < Tm: the time-major RNN input rows
 * (reference action_decoder_logistic.py:279-281) as the K-extension operand above. */
int tacorl_build_ad_input_bf16(const float* plan, const float* emb, int ld_emb, void* out_bf16, int B, int T, int Tm,
                               int P, int E, tacorl_stream_t stream);
/* BPTT step of the same RNN: y = (x Wt^T + addend) * [mask_src > 0], x = dZ_t (bf16), Wt = W_hh^T (bf16,
 * tacorl_transpose_to_bf16), addend = dH_{t-1}, mask_src = h_{t-1}; y fp32 + bf16 copy (next step's x). */
int tacorl_rnn_linear_bwd_step(const void* x_bf16, const void* wt_bf16, const float* addend, int ld_add,
                               const float* mask_src, float* y, void* y_bf16, int M, int K, int N,
                               tacorl_stream_t stream);
/* Weight gradient of the RNN's square matrices from the bf16 copies the ring GEMMs leave behind (replaces, for this
 * shape, tacorl_linear_wgrad's split-R slabs + reduce; reference: autograd of nn.RNN's weight_hh / weight_ih,
 * networks/action_decoders/rnn_models.py:5-16): dw[M][N] (+)= dz^T x, db[M] (+)= column sums of dz (db may be NULL).
 * dz bf16 [R][ld_dz], x bf16 [R][ld_x]; R % 64 == 0, M % 128 == 0, N % 128 == 0. */
int tacorl_rnn_wgrad_supported(int R, int M, int N);
int tacorl_rnn_wgrad(const void* dz_bf16, int ld_dz, const void* x_bf16, int ld_x, int R, int M, int N, float* dw,
                     float* db, int accumulate, tacorl_stream_t stream);
/* n <= 4 such gradients of one output shape in ONE launch (row counts R[p] may differ; db[p] may be NULL): the weight
 * gradients of nn.RNN's square matrices - weight_hh of every layer, weight_ih of the upper ones (reference rnn_models.py:5-16,
 * autograd) - behind the BPTT. */
int tacorl_rnn_wgrad_batch(int n, const void* const* dz_bf16, int ld_dz, const void* const* x_bf16, int ld_x, const int* R,
                           int M, int N, float* const* dw, float* const* db, int accumulate, tacorl_stream_t stream);
/* The same products for a FEW output rows and many reduction rows (the action decoder's 182 x H output heads): dz bf16
 * [R][ld_dz] with Mp >= rows columns in use (Mp % 128 == 0, columns >= rows zero), x bf16 [R][ld_x]; R is cut into `slabs` row
 * ranges (R % (64 slabs) == 0) that run side by side, a second launch sums the partial results in slab order into
 * dw[rows][N] / db[rows].  ws: tacorl_rnn_wgrad_slabs_ws_bytes(slabs, Mp, N). */
size_t tacorl_rnn_wgrad_slabs_ws_bytes(int slabs, int Mp, int N);
int tacorl_rnn_wgrad_slabs(const void* dz_bf16, int ld_dz, const void* x_bf16, int ld_x, int R, int Mp, int N, int rows,
                           int slabs, float* dw, float* db, int accumulate, void* ws, size_t ws_bytes, tacorl_stream_t stream);
/* The BPTT wavefront launch: nprob <= 4 problems y[p] = (x[p] Wt[p]^T + addend[p]) * [mask_src[p] > 0] (addend / mask
 * entries may be NULL) of one shape, fp32 y + optional bf16 copy: recurrent gradient steps of all layers and the
 * projection dH_{l-1}[t] = dZ_l[t] W_ih_l (Wt = W_ih_l^T) side by side (reference: autograd of nn.RNN, rnn_models.py:5-16). */
int tacorl_rnn_linear_bwd_batch(int nprob, const void* const* x_bf16, const void* const* wt_bf16,
                                const float* const* addend, int ld_add, const float* const* mask_src,
                                float* const* y, void* const* y_bf16, int M, int K, int N, tacorl_stream_t stream);
/* Row-order change between batch-major [n_outer][n_inner] and time-major [n_inner][n_outer] row blocks:
 * dst[(i*n_outer + o)][0..cols) = src[(o*n_inner + i)][0..cols).  The bidirectional ReLU-RNN plan recognition
 * (reference plan_encoders/plan_recognition_tanh_net.py, nn.RNN(num_layers=2, bidirectional=True)) runs its recurrence
 * over time-major slabs: its input embeddings come in and its input gradient goes out batch-major. */
int tacorl_birnn_swap_rows(const float* src, int ld_src, float* dst, int ld_dst, int n_outer, int n_inner, int cols,
                           tacorl_stream_t stream);
/* dst[c][r] = bf16(src[r][c]); R, C multiples of 32. */
int tacorl_transpose_to_bf16(const float* src, void* dst, int R, int C, tacorl_stream_t stream);
/* n <= 16 such transposes (dst[j][c][r] = bf16(src[j][r][c]), R[j] x C[j], multiples of 32) in ONE launch: the weights-only
 * preparation of the plan recognition's and the action decoder's backward (W^T operands of their input-gradient GEMMs;
 * autograd of nn.Linear / nn.RNN in the reference - plan_recognition_transformer.py:70-105, rnn_models.py:5-16). */
int tacorl_transpose_to_bf16_batch(int n, const float* const* src, void* const* dst, const int* R, const int* C,
                                   tacorl_stream_t stream);
/* dst[c][r] = r < R ? bf16(src[r][c]) : 0 for r < ld_dst (C, ld_dst multiples of 32): a weight whose row count is no multiple
 * of the ring GEMM's k-step as its K-padded transposed operand (the action decoder's 182 x H output heads, reference
 * action_decoder_logistic.py:44-52, in dH = d_heads W). */
int tacorl_transpose_pad_to_bf16(const float* src, void* dst, int R, int C, int ld_dst, tacorl_stream_t stream);
/* dst[r][c] = c < cols ? bf16(src[r][c]) : 0 for c < ld_dst (ld_dst % 8 == 0): a fp32 matrix as a K-padded bf16 operand. */
int tacorl_pad_to_bf16(const float* src, int ld_src, void* dst, int ld_dst, long rows, int cols, tacorl_stream_t stream);

/* Backward primitives of y = act(x W^T + b):
 *   dgrad: out[m][i] = (sum_o dz[m][o] W[o][i] + addend[m][i]) * act'(src[m][i])
 *   wgrad: dw[o][k] (+)= sum_m dz[m][o] x[m][k], db[o] (+)= sum_m dz[m][o]  (split-R slabs in ws). */
int tacorl_linear_dgrad(int nprob, const float* const* dz, int ld_dz, const float* const* w,
                        float* const* out, int ld_out, const float* const* src, int ld_src, int act_src,
                        const float* const* addend, int ld_add, const int* M, int O, int I,
                        int compute_dtype, tacorl_stream_t stream);
/* tacorl_linear_dgrad with the reduction split over workgroups (+ a reduce pass) when the output is skinny and O long;
 * falls back to the single-pass form when a src mask is given or ws is too small (tacorl_linear_dgrad_ws_bytes). */
size_t tacorl_linear_dgrad_ws_bytes(int nprob, const int* M, int O, int I);
int tacorl_linear_dgrad_splitk(int nprob, const float* const* dz, int ld_dz, const float* const* w,
                               float* const* out, int ld_out, const float* const* src, int ld_src, int act_src,
                               const float* const* addend, int ld_add, const int* M, int O, int I,
                               int compute_dtype, void* ws, size_t ws_bytes, tacorl_stream_t stream);
size_t tacorl_linear_wgrad_ws_bytes(int nprob, const int* M, int K, int O);
int tacorl_linear_wgrad(int nprob, const float* const* x, int ldx, const float* const* dz, int ld_dz,
                        const int* M, int K, int O, float* const* dw, float* const* db, int accumulate,
                        int compute_dtype, void* ws, size_t ws_bytes, tacorl_stream_t stream);
/* y = relu(conv2d(x, w) + b), no padding.  Replaces nn.Conv2d + nn.ReLU,
 * reference networks/visual_encoders/encoder.py:369-390. x_dtype: image storage dtype. */
int tacorl_conv2d_relu_fwd(int nprob, const void* const* x, const float* const* w,
                           const float* const* b, float* const* y, const int* n_img, int H, int W,
                           int C, int KH, int KW, int S, int CO, int x_dtype, int compute_dtype,
                           tacorl_stream_t stream);

/* ---- LMPVisionEncoder (reference encoder.py:349-419, utils.py:22-76) --------------- */
/* Packed parameter block (floats, every tensor 4-float aligned):
 *   0 conv1.w[32][8][8][3] 1 conv1.b 2 conv2.w[64][4][4][32] 3 conv2.b 4 conv3.w[64][3][3][64]
 *   5 conv3.b 6 temperature[1] 7 fc1.w[256][128] 8 fc1.b 9 fc2.w[32][256] 10 fc2.b
 * Writes the 11 offsets; returns the block size in floats. */
long tacorl_encoder_param_layout(long* offsets11);
/* Saved-activation block per problem: y1 | y2 | y3 | softargmax(128) | fc1(256). Writes the 5
 * offsets (floats), returns the block size in floats. */
long tacorl_encoder_act_layout(int n_img, int H, int W, long* offsets5);
int tacorl_encoder_fwd(int nprob, const void* const* img, const float* const* params,
                       float* const* out /*[n][32]*/, float* const* act, const int* n_img, int H,
                       int W, int img_dtype, int compute_dtype, tacorl_stream_t stream);
size_t tacorl_encoder_bwd_ws_bytes(int nprob, const int* n_img, int H, int W);
/* grads: blocks in the parameter layout (overwritten, or accumulated if accumulate != 0). */
int tacorl_encoder_bwd(int nprob, const void* const* img, const float* const* params,
                       const float* const* act, const float* const* d_out, float* const* grads,
                       const int* n_img, int H, int W, int img_dtype, int compute_dtype,
                       int accumulate, void* ws, size_t ws_bytes, tacorl_stream_t stream);

/* Fused inference forward (no saved activations): one launch, bf16 MFMA, register-stationary weights,
 * LDS-resident intermediates; bf16 NHWC images only; optionally saves the activations a backward needs.  `packed` = tacorl_encoder_pack_weights output
 * (tacorl_encoder_fused_wpk_bytes() bytes per network; re-pack whenever the fp32 block changes). */
long tacorl_encoder_fused_wpk_bytes(void);
int tacorl_encoder_fused_supported(int H, int W);
/* What the fused forward writes into a problem's act block for this geometry: 0 - not a fused geometry; 1 - y1 / y2 as bf16 at
 * the start of their slots (tacorl_encoder_bwd_fused* read them); 2 - every activation as fp32, i.e. exactly what the per-layer
 * tacorl_encoder_fwd leaves and tacorl_encoder_bwd reads (a geometry of csrc/encoder_ring.hip - conv1 output too large for the
 * LDS - for which tacorl_encoder_bwd_fused_ws_bytes() is 0.  150 x 200, the un-resized rgb_static of the reference's
 * experiment=tacorl_real_world, config/.../rl_real_world_train.yaml:2-10, has the LDS-resident backward and reports 1). */
int tacorl_encoder_fused_act_format(int H, int W);
int tacorl_encoder_pack_weights(int nprob, const float* const* params, void* const* packed,
                                tacorl_stream_t stream);
/* act: NULL, or per-problem pointers (NULL entries allowed) to tacorl_encoder_act_layout blocks that
 * receive the fp32 activations tacorl_encoder_bwd needs.  Saved activations (act[p] != NULL, layout of
 * tacorl_encoder_act_layout): y3, the soft-argmax features and fc1 as fp32; y1 and y2 as **bf16** at the start of their
 * fp32-sized slots - the values the next layer consumed - which is what tacorl_encoder_bwd_fused* read (geometries of
 * tacorl_encoder_fused_act_format() == 2: all five as fp32, for tacorl_encoder_bwd). */
int tacorl_encoder_fwd_fused(int nprob, const void* const* img, const void* const* packed,
                             const float* const* params, float* const* out, float* const* act,
                             const int* n_img, int H, int W, tacorl_stream_t stream);
/* The same launch on at most max_workgroups workgroups (0 = one per CU): fewer than the CU count leaves CUs to a concurrent
 * branch of the caller's graph - TACORL issues the frozen LMP window's problems first, forks the plan recognition ->
 * action decoder branch (reference tacorl.py:142-179, 206-233: neither depends on the actor / critic encoders) and runs the
 * update's own encoder problems beside it on 160 workgroups.  The launch is shared out by WORK UNITS (an image costs 64, or 72
 * with saved activations; a workgroup may serve the tail of one problem and the head of the next): which workgroup serves
 * which image changes nothing in the results.  max_workgroups, when given, must be at least nprob (TACORL_EINVAL otherwise). */
int tacorl_encoder_fwd_fused_wg(int nprob, const void* const* img, const void* const* packed,
                                const float* const* params, float* const* out, float* const* act,
                                const int* n_img, int H, int W, int max_workgroups, tacorl_stream_t stream);
/* The same launch with a source per problem: src NULL or src[p] NULL - the packed bf16 NHWC images at img[p]; otherwise src[p]
 * is the DEVICE address of a table entry (tacorl_encoder_src_entry_bytes() each, written by tacorl_encoder_src_fill) that
 * names n_img[p] contiguous fp32 CHW images, image i at base + i * img_pitch floats.  The kernel converts them itself (round
 * to nearest even, as tacorl_pack_images*) while it computes the image before: out is bit-identical to the packed route.  The
 * entry is read when the kernel RUNS, so a captured launch follows whatever the last fill named.  84 x 84 only, never with
 * act[p] (a backward reads the packed image): TACORL_EINVAL otherwise.  tacorl_encoder_src_supported: would fill accept it? */
long tacorl_encoder_src_entry_bytes(void);
int tacorl_encoder_src_supported(const float* base, long img_pitch, long plane_pitch, long row_pitch, int H, int W);
int tacorl_encoder_src_fill(void* table, int n, const float* const* base, const long* img_pitch, const long* plane_pitch,
                            const long* row_pitch, int H, int W, tacorl_stream_t stream);
int tacorl_encoder_fwd_fused_src(int nprob, const void* const* img, const void* const* src, const void* const* packed,
                                 const float* const* params, float* const* out, float* const* act, const int* n_img, int H,
                                 int W, int max_workgroups, tacorl_stream_t stream);

/* Backward twin of the fused forward (same preconditions: bf16 NHWC images, bf16 MFMA, a geometry
 * tacorl_encoder_fused_supported() accepts; at most 4 problems): FC tail and soft-argmax as
 * tacorl_encoder_bwd, the three convolutions' dgrad/wgrad as per-image LDS-resident kernels. Same
 * argument meaning as tacorl_encoder_bwd. Replaces autograd through
 * networks/vision/lmp_vision_network.py:32-66. */
size_t tacorl_encoder_bwd_fused_ws_bytes(int nprob, const int* n_img, int H, int W);
int tacorl_encoder_bwd_fused(int nprob, const void* const* img, const float* const* params,
                             const float* const* act, const float* const* d_out,
                             float* const* grads, const int* n_img, int H, int W, int accumulate,
                             void* ws, size_t ws_bytes, tacorl_stream_t stream);
/* The same backward in parts that share `ws`, so that a caller can keep only the dependent chain on its
 * main stream:  _pack (weight-only preparation: any time after the last optimiser step) -> _head (FC tail
 * input-gradient chain, one launch) -> _conv (soft-argmax + conv backward); _fc_wgrad (FC weight
 * gradients) may run on another stream any time after _head.  prepacked = 1: _pack already ran for the
 * current weights. */
int tacorl_encoder_bwd_fused_pack(int nprob, const float* const* params, const int* n_img, int H, int W,
                                  void* ws, size_t ws_bytes, tacorl_stream_t stream);
int tacorl_encoder_bwd_fused_head(int nprob, const float* const* params, const float* const* act,
                                  const float* const* d_out, const int* n_img, int H, int W,
                                  int prepacked, void* ws, size_t ws_bytes, tacorl_stream_t stream);
int tacorl_encoder_bwd_fused_fc_wgrad(int nprob, const float* const* act, const float* const* d_out,
                                      float* const* grads, const int* n_img, int H, int W,
                                      int accumulate, void* ws, size_t ws_bytes, tacorl_stream_t stream);
int tacorl_encoder_bwd_fused_conv(int nprob, const void* const* img, const float* const* params,
                                  const float* const* act, float* const* grads, const int* n_img, int H,
                                  int W, int accumulate, int prepacked, void* ws, size_t ws_bytes,
                                  tacorl_stream_t stream);
/* The same, a subset of its launches (parts, a bit mask: 1 soft-argmax backward, 2 dgrad3, 4 wgrad3, 8 dgrad2,
 * 16 wgrad2, 32 wgrad1, 64 slab reduce; 127 = all), so that a caller can put the weight gradients of conv3 / conv2 on a
 * second stream beside the dgrad3 -> dgrad2 -> wgrad1 chain.  The caller orders the streams: dgrad2 and wgrad2 read
 * dgrad3's output, wgrad1 reads dgrad2's, the reduce reads every wgrad's slabs.  Partial calls need prepacked = 1 (TACORL_EINVAL otherwise,
 * before anything is launched - the soft-argmax backward of the same call included). */
int tacorl_encoder_bwd_fused_conv_parts(int nprob, const void* const* img, const float* const* params,
                                        const float* const* act, float* const* grads, const int* n_img, int H,
                                        int W, int accumulate, int prepacked, int parts, void* ws,
                                        size_t ws_bytes, tacorl_stream_t stream);

/* ---- MLP = chain of Linear(dims[l] -> dims[l+1]) + acts[l]  ------------------------ */
/* Parameter block: for each layer W[out][in] then b[out], each 4-float aligned. */
long tacorl_mlp_param_layout(int n_layers, const int* dims, long* w_off, long* b_off);
/* Activation block for M rows: per layer [z_l if SiLU][y_l]; y_off[n_layers-1] is the output. */
long tacorl_mlp_act_layout(int M, int n_layers, const int* dims, const int* acts, long* z_off,
                           long* y_off);
int tacorl_mlp_fwd(int nprob, const float* const* x, int ldx, const float* const* params,
                   float* const* act, const int* M, int n_layers, const int* dims,
                   const int* acts, int compute_dtype, tacorl_stream_t stream);
/* The same forward as ONE launch (bf16 MFMA only; <= 8 problems, <= 4 layers, every layer input width a
 * multiple of 8 and all widths <= 256, ldx % 4 == 0 - query with _supported).  params_bf16[p] is a bf16
 * copy of params[p] at the same element offsets (tacorl_to_bf16_batch); the caller refreshes it
 * whenever the fp32 block changes.  Saved activations are identical in layout to tacorl_mlp_fwd's.  An unsupported
 * shape or a misaligned x / params (16 bytes) / params_bf16 (8 bytes) of ANY problem is refused with TACORL_EINVAL before
 * anything is launched. */
int tacorl_mlp_fwd_fused_supported(int nprob, int n_layers, const int* dims, int ldx);
/* lean != 0: hidden-layer outputs whose pre-activation is saved are not written; the fused weight-gradient launch
 * (same flag) recomputes them.  Only where tacorl_mlp_lean_supported() - forward, input-gradient chain and one-launch
 * weight gradients all fused - and nothing else reads those hidden outputs. */
int tacorl_mlp_lean_supported(int nprob, int n_layers, const int* dims, int ldx, int ldo, int ldd);
int tacorl_mlp_fwd_fused(int nprob, const float* const* x, int ldx, const float* const* params,
                         const void* const* params_bf16, float* const* act, const int* M,
                         int n_layers, const int* dims, const int* acts, int lean, tacorl_stream_t stream);
/* tacorl_mlp_fwd_fused with a GATHERED layer-0 input: row r of problem p is the concatenation of nseg[p] <= 4 column
 * segments; segment t supplies columns [seg_c0[4p+t], seg_c0[4p+t+1]) (the last one up to dims[0]) from
 * seg_ptr[4p+t][(seg_mod[4p+t] ? r % seg_mod[4p+t] : r) * seg_ld[4p+t] + col - seg_c0[4p+t]].  This is the reference's
 * torch.cat([enc(obs), goal_enc(enc(goal))]) (networks/actor_critic/visual_actor_wrapper.py:41-62,
 * visual_critic_wrapper.py:50-71), torch.cat([emb, action]) (critic.py:92-97) and expand_obs (utils/misc.py:132-153:
 * state rows repeated for every sampled action = seg_mod B) read where the producers left them, with no copy launch in
 * front of the MLP.  x_out != NULL and x_out[p] != NULL: the assembled fp32 rows are also written to x_out[p] ([M][ldx]),
 * layer 0's operand of the weight-gradient launch.  seg_c0 % 8 == 0, seg_ld % 4 == 0, pointers 16-byte aligned.
 * _supported == 0 (a many-row problem of a lean site, or shapes the fused forward does not take): assemble with
 * tacorl_copy_cols_batch and call tacorl_mlp_fwd_fused / tacorl_mlp_fwd. */
int tacorl_mlp_fwd_fused_gather_supported(int nprob, const int* M, int n_layers, const int* dims, const int* acts,
                                          int ldx, int lean);
int tacorl_mlp_fwd_fused_gather(int nprob, const int* nseg, const float* const* seg_ptr, const int* seg_ld,
                                const int* seg_c0, const int* seg_mod, float* const* x_out, int ldx,
                                const float* const* params, const void* const* params_bf16, float* const* act,
                                const int* M, int n_layers, const int* dims, const int* acts, int lean,
                                tacorl_stream_t stream);
/* tacorl_mlp_fwd_fused_gather that also writes, for problems with xb_out[p] != NULL, the weight gradients' layer-0 operand:
 * the input rows as bf16 [Mp][128] (Mp = M rounded up to 64), zeros beyond dims[0] columns and beyond M rows - the copy
 * tacorl_mlp_bwd_fused_wgrad otherwise converts from x with a launch of its own.  xb_out[p] = the backward site's workspace +
 * tacorl_mlp_bwd_fused_xb_offset(...) (-1: problem p of that site has no such region); the site's _wgrad call then passes
 * lean | 2.  Only for problems of a lean site with 2048 <= M < 16384 rows; TACORL_EINVAL otherwise. */
int tacorl_mlp_fwd_fused_gather_xb(int nprob, const int* nseg, const float* const* seg_ptr, const int* seg_ld,
                                   const int* seg_c0, const int* seg_mod, float* const* x_out, void* const* xb_out, int ldx,
                                   const float* const* params, const void* const* params_bf16, float* const* act,
                                   const int* M, int n_layers, const int* dims, const int* acts, int lean,
                                   tacorl_stream_t stream);
long tacorl_mlp_bwd_fused_xb_offset(int nprob, const int* M, int n_layers, const int* dims, int p);
/* dst[i][:] = bf16(src[i][:]) for n <= 16 buffers in one launch (count[i] % 4 == 0). */
int tacorl_to_bf16_batch(int n, const float* const* src, void* const* dst, const long* count,
                         tacorl_stream_t stream);
size_t tacorl_mlp_bwd_ws_bytes(int nprob, const int* M, int n_layers, const int* dims);
/* d_out: gradient w.r.t. the last layer's output [M][dims[n_layers]], leading dim ldo (last act
 * NONE, or TANH: d_out is then multiplied by 1 - y^2 of the saved output first).
 * grads[p] may be NULL (skip weight gradients); d_x[p] may be NULL (skip input gradient). */
int tacorl_mlp_bwd(int nprob, const float* const* x, int ldx, const float* const* params,
                   const float* const* act, const float* const* d_out, int ldo, float* const* grads,
                   float* const* d_x, int ldd, const int* M, int n_layers, const int* dims,
                   const int* acts, int compute_dtype, int accumulate, void* ws, size_t ws_bytes,
                   tacorl_stream_t stream);
/* bf16 mode, <= 8 problems, <= 4 layers, widths <= 256: the backward split in two calls that share `ws`.
 *   _dgrad: the whole input-gradient chain dZ_{l-1} = (dZ_l W_l) * act'_{l-1} in ONE launch (plus a weight
 *           transpose launch); leaves every dZ_l in ws and writes d_x[p] (NULL = not wanted).
 *   _wgrad: weight / bias gradients from those dZ_l (grads[p] NULL = skip the problem); may run on
 *           another stream once _dgrad has finished - it is not on the dependent chain of the step.
 * Together they equal tacorl_mlp_bwd (autograd through the Linear/SiLU/ReLU stacks of
 * networks/actor_critic/{actor,critic}.py and visual_encoders/goal_encoder.py). */
int tacorl_mlp_bwd_fused_supported(int nprob, int n_layers, const int* dims, int ldo, int ldd);
size_t tacorl_mlp_bwd_fused_ws_bytes(int nprob, const int* M, int n_layers, const int* dims);
/* prepacked: bit 0 = weight transposes already in ws (tacorl_mlp_bwd_fused_pack); bit 1 = this MLP site runs lean
 * (tacorl_mlp_fwd_fused and _wgrad with lean != 0): at >= 16 384 rows (C5's Q networks: 99 328) the forward then also
 * leaves bf16 copies of the hidden outputs, _dgrad leaves its dZ_l as bf16, and _wgrad streams both by LDS-DMA
 * (mlp_wgrad_big_kernel) - the three calls must agree on the flag. */
int tacorl_mlp_bwd_fused_dgrad(int nprob, const float* const* params, const float* const* act,
                               const float* const* d_out, int ldo, float* const* d_x, int ldd,
                               const int* M, int n_layers, const int* dims, const int* acts,
                               int prepacked, void* ws, size_t ws_bytes, tacorl_stream_t stream);
/* The weight transposes _dgrad needs, alone (they depend only on the parameters: run them early / on
 * another stream, then pass prepacked = 1 to _dgrad). */
int tacorl_mlp_bwd_fused_pack(int nprob, const float* const* params, const int* M, int n_layers,
                              const int* dims, void* ws, size_t ws_bytes, tacorl_stream_t stream);
/* Weight-only preparation of a step as ONE launch.  Between _begin() and _end(stream) - same host thread - the entry
 * points whose launches read nothing but parameters (tacorl_to_bf16_batch, tacorl_mlp_bwd_fused_pack and the FC-tail
 * transposes of tacorl_encoder_bwd_fused_pack) only record their jobs; _end issues them together on `stream`, which must
 * be the stream those calls were given.  Replaces, in the reference's terms, nothing: torch.nn.Linear's backward
 * (networks/actors/actor.py:28-60, critics/critic.py:92-97 via autograd) has no such step - the transposed bf16 copies
 * are this implementation's MFMA operands.  _begin inside an open batch and _end without one return TACORL_EINVAL. */
int tacorl_prep_batch_begin(void);
/* The same for the slab reduces that finish the one-launch MLP weight gradients (tacorl_mlp_bwd_fused_wgrad,
 * tacorl_encoder_bwd_fused_fc_wgrad): between tacorl_reduce_batch_begin() and _end(stream) they are recorded, and _end
 * sums every site's slabs in one launch - the gradients are complete only after _end.  Their only readers are the
 * gradient all-reduce and the optimiser (reference cql_offline_lightning.py:519-542: the three optimizer.step() calls). */
int tacorl_reduce_batch_begin(void);
int tacorl_reduce_batch_end(tacorl_stream_t stream);
int tacorl_prep_batch_end(tacorl_stream_t stream);
/* lean: bit 0 = the site runs lean (above); bit 1 = the many-row problems' bf16 input rows in ws are current - the forward
 * wrote them (tacorl_mlp_fwd_fused_gather_xb) - so x is not converted again.  Bit 1 for a region no such forward was given
 * (with this M, on this host thread) since the last _wgrad call over it is TACORL_EINVAL: every _wgrad call uses the note up.
 * This guards against a bit set without the address having been passed; it tracks addresses, not the bytes behind them. */
int tacorl_mlp_bwd_fused_wgrad(int nprob, const float* const* x, int ldx, const float* const* act,
                               const float* const* d_out, int ldo, float* const* grads, const int* M,
                               int n_layers, const int* dims, const int* acts, int accumulate, int lean,
                               void* ws, size_t ws_bytes, tacorl_stream_t stream);

/* ---- data movement ----------------------------------------------------------------- */
/* n images (image i at src + i*img_pitch floats; NCHW if src_nchw else NHWC) -> contiguous NHWC
 * dst (fp32 / bf16).  Replaces the states[:,0] / states[:,-1] / goal gathers of
 * TACORL.get_rl_batch (reference modules/tacorl/tacorl.py:142-179). */
int tacorl_pack_images(const float* src, long img_pitch, int src_nchw, void* dst, int dst_dtype,
                       int n, int C, int H, int W, tacorl_stream_t stream);
/* Up to 8 NCHW (C = 3, H*W % 4 == 0, 16-byte aligned) -> NHWC packs in one launch: the B*T window frames
 * and the obs / goal / next-obs images of a TACORL step (reference get_rl_batch, tacorl.py:142-179). */
int tacorl_pack_images_batch(int njobs, const float* const* src, const long* img_pitch, void* const* dst,
                             const int* n_img, int dst_dtype, int H, int W, tacorl_stream_t stream);
/* The same with second destinations for WINDOW jobs (window[j] = T >= 2, n_img[j] % T == 0): image i = b T + t of job j is
 * also written to image b of dst_first[j] (t == 0) or of dst_last[j] (t == T - 1).  TACO-RL's transition (s, s') is the
 * window's first and last frame (reference modules/tacorl/tacorl.py:147-168, get_rl_batch), so the step's obs / next
 * images are packed from the one read of the window instead of being read again: 2 B of 19 B fp32 frames per step.
 * window == NULL or window[j] == 0: a plain job. */
int tacorl_pack_images_window_batch(int njobs, const float* const* src, const long* img_pitch, void* const* dst,
                                    const int* n_img, void* const* dst_first, void* const* dst_last,
                                    const int* window, int dst_dtype, int H, int W, tacorl_stream_t stream);
/* The dataset's own frame format: uint8 HWC (reference datamodule/dataset/play_dataset.py) -> NHWC fp32 / bf16 with the
 * reference's transform pipeline applied on the way, ToTensor (x / 255) and Normalize(0.5, 0.5) ((t - 0.5) / 0.5) in
 * fp32 (config .../rl_train.yaml:12-14): bit-identical to packing the transformed fp32 frames, a quarter of the
 * bytes read.  Jobs as in tacorl_pack_images_batch; pitches in bytes; H*W*3 % 16 == 0, 16-byte aligned. */
int tacorl_pack_images_u8_batch(int njobs, const void* const* src, const long* img_pitch_bytes, void* const* dst,
                                const int* n_img, int dst_dtype, int H, int W, tacorl_stream_t stream);
/* The same pack reading its images BY FRAME INDEX out of a uint8 dataset resident in device (or mapped host) memory:
 * image i of job j is frame index[j][i * index_stride[j]] of the dataset at src[j] (pitch = bytes per frame); index[j]
 * NULL = image i (the plain pack).  One pass from the replay store into the encoder's image buffers - the window
 * frames (stride 1) and the obs / goal / next images (strides T, 1, T over the same id table) of a TACORL step -
 * instead of a gather into a uint8 batch followed by the pack (reference datamodule/dataset/play_dataset.py:115-169,
 * 357-419 assembles the window on the host).  Ids are NOT range-checked here: tacorl_amd/data/replay.py checks them. */
int tacorl_pack_images_u8_gather_batch(int njobs, const void* const* src, const long* img_pitch_bytes,
                                       const long* const* index, const int* index_stride, void* const* dst,
                                       const int* n_img, int dst_dtype, int H, int W, tacorl_stream_t stream);
/* Replay data path on the GPU.
 * tacorl_gather_frames_u8: dst[i] = frames[index[i]] - a step's window / goal frames out of the uint8 HWC dataset
 * resident in HBM (reference datamodule/dataset/play_dataset.py:357-419 loads them from per-frame .npz files);
 * frame_bytes % 16 == 0, index: device int64[n].
 * tacorl_pack_images_u8_aug_batch: the reference's train-time image pipeline on the way into the NHWC image
 * buffers (config/datamodule/transform_manager/transforms/rl_train.yaml): RandomShiftsAug (utils/transforms.py:
 * 265-299; shift[i] = (sx, sy) in [0, 2*pad], the reference's randint draw - an integer shift of the replicate-padded
 * frame), x/255, torchvision ColorJitter (utils/transforms.py:302-330; jitter[i] = {brightness factor, contrast
 * factor, hue shift, the 4 drawn positions of fn_idx (0 brightness, 1 contrast, 2 saturation = unused, 3 hue),
 * apply flag}), Normalize(0.5, 0.5).  shift / jitter: device tables per job, NULL (array or entry) = that stage off. */
int tacorl_gather_frames_u8(const void* frames, long frame_bytes, const long* index, void* dst, long n,
                            tacorl_stream_t stream);
int tacorl_pack_images_u8_aug_batch(int njobs, const void* const* src, const long* img_pitch_bytes,
                                    void* const* dst, const int* const* shift, const float* const* jitter,
                                    const int* n_img, int dst_dtype, int H, int W, int pad,
                                    tacorl_stream_t stream);
/* The whole train pipeline of rl_train.yaml including its first stage, torchvision.transforms.Resize (:3-4,16-17: the
 * 200x200 camera frames -> 128x128 static / 84x84 gripper): source frames src_H x src_W uint8 HWC (pitch = bytes per
 * source frame), bilinear with align_corners = False and no antialias on the 0..255 values - what torchvision's
 * tensor path computes through torch.nn.functional.interpolate - then RandomShiftsAug on the H x W result, x/255,
 * ColorJitter, Normalize.  src_H == H and src_W == W: no resize (tacorl_pack_images_u8_aug_gather_batch). */
int tacorl_pack_images_u8_resize_aug_gather_batch(int njobs, const void* const* src, const long* img_pitch_bytes,
                                                  const long* const* index, const int* index_stride, void* const* dst,
                                                  const int* const* shift, const float* const* jitter, const int* n_img,
                                                  int dst_dtype, int src_H, int src_W, int H, int W, int pad,
                                                  tacorl_stream_t stream);
/* The Resize stage alone, at store time (csrc/frame_ops.hip; the dataset key `store_size` of the frame datamodules): n uint8
 * HWC frames of src_H x src_W, src_pitch_bytes apart -> n uint8 HWC frames of H x W, dst_pitch_bytes apart.  The same
 * sampling arithmetic in the same order as the pack above (one device function, csrc/bilinear.h), then round to nearest
 * even, clamp to 0..255, store.  src_H == H and src_W == W copies.  Bytes between a frame's end and the next frame are
 * neither read into a result nor written.  TACORL_EINVAL before any launch: a null pointer, src or dst not 16-byte aligned,
 * n or a size < 1, a pitch smaller than its frame, or a source so wide that the rows one band of 16 output rows samples
 * exceed 48 KB of LDS ((15 * src_H / H + 4) * src_W * 3 bytes).  Never allocates. */
int tacorl_resize_frames_u8(const void* src, long src_pitch_bytes, void* dst, long dst_pitch_bytes, long n, int src_H,
                            int src_W, int H, int W, tacorl_stream_t stream);
/* ... and the augmenting pack with the same optional frame-index tables (shift / jitter tables are per IMAGE i). */
int tacorl_pack_images_u8_aug_gather_batch(int njobs, const void* const* src, const long* img_pitch_bytes,
                                           const long* const* index, const int* index_stride, void* const* dst,
                                           const int* const* shift, const float* const* jitter, const int* n_img,
                                           int dst_dtype, int H, int W, int pad, tacorl_stream_t stream);
/* reward = done = float(disp == 1) (done may be NULL) and acts_dst[0:n_acts] = acts_src[0:n_acts], one launch:
 * the small tensors of TACORL.get_rl_batch (reference modules/tacorl/tacorl.py:142-179).
 * disp_dtype: 0 float32, 1 int64, 2 int32, 3 uint8 / bool. */
int tacorl_stage_transition(const void* disp, int disp_dtype, float* reward, float* done, int B,
                            const float* acts_src, float* acts_dst, long n_acts, tacorl_stream_t stream);
/* TACORL's step front on its fp32-source route as ONE launch over a device-resident table at a fixed address: per camera the
 * fused encoder's source entries [window | next] (the layout of tacorl_encoder_src_fill's entries; camera i's are entries
 * 2 i and 2 i + 1 at offsets[0] + k * tacorl_encoder_src_entry_bytes()), the pack jobs [obs; goal] of the engine cameras
 * (fp32 CHW -> bf16 NHWC, bit-identical to tacorl_pack_images_batch) and tacorl_stage_transition's sources and destinations.
 *   tacorl_step_front_table_bytes / _offsets: the table's size and the byte offsets of its TACORL_SF_NOFFSETS fields, in the
 *     order src, pack_src, pack_dst, pack_pitch, pack_n, disp, reward, done, acts_src, acts_dst, n_acts, disp_dtype, B,
 *     njobs, HW.
 *   tacorl_step_front_supported (pure host): sources as tacorl_encoder_src_supported takes them (contiguous 84 x 84 images,
 *     pitches in floats), pack jobs 16-byte aligned at both ends with pitch % 4 == 0 and n >= 1, H*W % 4 == 0, a disp dtype
 *     code of tacorl_stage_transition, B >= 1, at most 2 * TACORL_SF_MAXCAM sources and TACORL_SF_MAXJOBS jobs.
 *   tacorl_step_front_assemble (pure host): the table's bytes for these entries into host_table (unused entries and padding
 *     zero, so equal entries give equal bytes: the caller keeps them as the shadow of the device table and skips the fill
 *     while they do not change); TACORL_EINVAL, nothing written, for what _supported refuses.
 *   tacorl_step_front_fill: one small launch writes assembled bytes (passed by value) over the device table.
 *   tacorl_step_front: blockIdx.y < njobs packs job blockIdx.y, the last blockIdx.y stages the transition.  The table is read
 *     when the kernel RUNS: a captured launch follows the batch tensors the last fill named.  njobs, max_images (the largest
 *     job), B, n_acts, H, W size the grid and must be the filled table's. */
#define TACORL_SF_MAXCAM 4
#define TACORL_SF_MAXJOBS 8
#define TACORL_SF_NOFFSETS 15
long tacorl_step_front_table_bytes(void);
int tacorl_step_front_offsets(long* offsets);
int tacorl_step_front_supported(int nsrc, const float* const* src_base, const long* src_pitch, int njobs,
                                const float* const* pack_src, const long* pack_pitch, void* const* pack_dst,
                                const int* pack_n, const void* disp, int disp_dtype, const float* reward, int B,
                                const float* acts_src, const float* acts_dst, long n_acts, int H, int W);
int tacorl_step_front_assemble(void* host_table, int nsrc, const float* const* src_base, const long* src_pitch, int njobs,
                               const float* const* pack_src, const long* pack_pitch, void* const* pack_dst,
                               const int* pack_n, const void* disp, int disp_dtype, float* reward, float* done, int B,
                               const float* acts_src, float* acts_dst, long n_acts, int H, int W);
int tacorl_step_front_fill(void* table, const void* host_table, tacorl_stream_t stream);
int tacorl_step_front(const void* table, int njobs, int max_images, int B, long n_acts, int H, int W,
                      tacorl_stream_t stream);
/* The transition sampler of CQL_Offline's dataset (reference datamodule/dataset/goal_cond_replay_buffer_dataset.py:
 * 145-299) over resident tables, one thread per sample b < B:
 *   step = possible_steps[idx[b]], end = ep_end[k] of the last episode with ep_start[k] <= step (binary search), and by
 *   strategy[b]: 0 geometric      goal = min(end, step + disp[b])
 *                1 similar_robot_obs  goal = nn_val[nn_ptr[step] + floor(u * count)] (CSR over steps [0, n_nn)); an empty
 *                                 or missing list falls back to `random`
 *                2 random         goal = possible_steps[j + (j >= idx[b])], j = floor(u * (n_possible - 1))
 *                3 increasing_horizon  goal = step + 1 + floor(u * (min(end, step + current_horizon) - step))
 *                4 episode_future goal = step + 1 + floor(u * (end - step))
 *                5 next_state     goal = step + 1
 *   with u = u_choice[b] in [0, 1).  ids: int64 (3, B) = [step | step + 1 | goal] (the id tables of the obs / next / goal
 *   image packs, stride 1 at offsets 0, B, 2B); action[b] = actions[step] (A floats); reward[b] = done[b] = (goal == step+1).
 * The tables are validated by the host (tacorl_amd/data/replay.py TransitionIndex) and every id they can produce lies in
 * [0, n_frames); each id is nevertheless clamped to that range before it is written, and *status is set to 1 (it is never
 * cleared here) when a clamp changed a value, idx[b] lay outside [0, n_possible) or strategy[b] is none of the above.
 * All pointers are device pointers, 8-byte (int64 / double) or 4-byte (float / int) aligned; nn_ptr / nn_val may be
 * NULL when n_nn == 0.  Nothing is allocated; B <= 0, A <= 0, an empty table or a NULL / misaligned pointer is refused
 * with TACORL_EINVAL before anything is launched. */
int tacorl_sample_transitions(const long* possible_steps, long n_possible, const long* ep_start, const long* ep_end,
                              int n_episodes, const long* nn_ptr, long n_nn, const long* nn_val, const float* actions,
                              const long* idx, const long* strategy, const long* disp, const double* u_choice,
                              long current_horizon, long n_frames, int B, int A, long* ids, float* action,
                              float* reward, float* done, int* status, tacorl_stream_t stream);
/* The sampler of RelayImitationLearning's dataset (reference datamodule/dataset/relay_imitation_learning_dataset.py:73-113)
 * over resident tables, one thread per sample b < B (256 threads per block), with Lw = max_low_level_window and
 * Hw = max_high_level_window:
 *   step = episode_lookup[idx[b]], end = ep_end[k] of the last episode with ep_start[k] <= step (binary search),
 *   sub  = min(end, step + Lw)                      (the subgoal frame, `high_level_action`)
 *   low  = step + 1 + floor(u_low[b] * (sub - step - 1))   where sub - step - 1 > 0, else sub
 *   hmax = min(end, step + Hw)
 *   high = sub + floor(u_high[b] * (hmax - sub))           where hmax - sub > 0, else hmax   (hmax < sub when Hw < Lw)
 *   with u in [0, 1), the floors kept inside their ranges, and the two minima formed without the overflow of a huge window.
 *   ids: int64 (4, B) = [step | low | high | sub] - obs, low_level_goal, high_level_goal, high_level_action, the id tables
 *   of the four image packs (stride 1 at offsets 0, B, 2B, 3B); action[b] = actions[step] (A floats).
 * The tables are validated by the host (tacorl_amd/data/relay_replay.py RelayIndex) and every id they can produce lies in
 * [0, n_frames); idx[b] is nevertheless clamped into [0, n_items) before the lookup is read, step and end into the dataset
 * before they are used, and each id into [0, n_frames) before it is written; *status is set to 1 (it is never cleared here)
 * when a clamp changed a value.  All pointers are device pointers, 8-byte (int64 / double) or 4-byte (float / int) aligned.
 * Nothing is allocated; a non-positive B, A, n_items, n_episodes, n_frames or window, or a NULL / misaligned pointer, is
 * refused with TACORL_EINVAL before anything is launched. */
int tacorl_sample_relay(const long* episode_lookup, long n_items, const long* ep_start, const long* ep_end, int n_episodes,
                        const float* actions, long n_frames, const long* idx, const double* u_low, const double* u_high,
                        long max_low_level_window, long max_high_level_window, int B, int A, long* ids, float* action,
                        int* status, tacorl_stream_t stream);
/* The window sampler of the vector-observation dataset (reference datamodule/dataset/d4rl_play_dataset.py:69-146) over
 * resident tables, one 64-lane wavefront per window b < B (four windows per block, grid ceil(B / 4)):
 *   s = episode_lookup[idx[b]], ws = window[b] in [min_window, Tmax];
 *   obs[b] (Tmax, S) = observations[s : s + ws], then the window's last row repeated; act[b] (Tmax, A) = actions[s : s + ws],
 *   then zero rows; and with G > 0 (G = 2 for AntMaze; G = 0: no goal, disp is not read):
 *   end = ep_end[k] of the last episode with ep_start[k] <= s (binary search), goal_step = min(end, s + (ws - 1) * disp[b])
 *   decided without forming a product that could overflow, goal[b] = observations[goal_step][0:G],
 *   reached[b] = done[b] = (sqrtf(dx*dx + dy*dy) < threshold ? 1 : 0) in fp32 with (dx, dy) = goal[b][0:2] -
 *   observations[s + ws - 1][0:2].  window_size (B) int64 = ws; ids (2, B) int64 = [s | goal_step] (goal_step = s when G = 0).
 * goal, reached, done, window_size and ids may each be NULL (not written).  The tables are validated by the host
 * (tacorl_amd/data/d4rl_replay.py D4RLWindowIndex) and every id they can produce lies in [0, n_frames); idx, window, disp
 * (>= 1), s and goal_step are nevertheless clamped into range before any table access, and *status is set to 1 (it is never
 * cleared here) when a clamp changed a value.  All pointers are device pointers, 8-byte (int64) or 4-byte (float / int)
 * aligned.  Nothing is allocated; a non-positive size, G == 1 or G > S, min_window outside [1, Tmax], n_frames < Tmax or a
 * NULL required / misaligned pointer is refused with TACORL_EINVAL before anything is launched. */
int tacorl_sample_d4rl_windows(const long* episode_lookup, long n_items, const long* ep_start, const long* ep_end,
                               int n_episodes, const float* observations, const float* actions, long n_frames,
                               const long* idx, const long* window, const long* disp, int B, int Tmax, int S, int A,
                               int G, int min_window, float threshold, float* obs, float* act, float* goal,
                               float* reached, float* done, long* window_size, long* ids, int* status,
                               tacorl_stream_t stream);
/* The play-window sampler (reference datamodule/dataset/play_dataset.py:115-169,258-310; PlayIndex.sample + pad_actions of
 * tacorl_amd/data/replay.py) over resident tables, one 64-lane wavefront per window b < B (four windows per block, grid
 * ceil(B / 4)):
 *   s = episode_lookup[idx[b]], ws = window[b] in [min_window, Tmax], end = ep_end[k] of the last episode with
 *   ep_start[k] <= s (binary search; -1 where s lies in no episode), rs = episode_lookup[min(floor(u_random_state[b] *
 *   n_items), n_items - 1)] (the random state);
 *   strategy[b] == 0 (geometric): goal = min(end, s + (ws - 1) * disp[b] + noise_step[b]) decided without forming a product
 *     that could overflow (a one-frame window has stride 0 and is not divided by), rs where end < 0; noise_step NULL: 0;
 *   strategy[b] == 1 (similar_robot_obs): with key = s + ws - 1 and cnt = nn_ptr[key + 1] - nn_ptr[key] (0 where key lies
 *     outside [0, n_nn)): goal = nn_val[nn_ptr[key] + min(floor(u_choice[b] * cnt), cnt - 1)] where cnt > 0, else rs;
 *   goal is then clipped into [0, last_end] (last_end = max(ep_end); part of the definition, it raises no status); the
 *   products u * n are formed in double and truncated, as NumPy does.
 *   ids: int64 (B * Tmax + B) = the window's frame ids s + min(t, ws - 1), row-major (b, t), then the B goal ids (the id table
 *   of the window / goal image packs); act (B, Tmax, A) = actions[s : s + ws], then rows that are zero except the last column
 *   (the gripper action), which repeats the last real step's; disp_out (B) = disp[b] for a geometric goal, else -1;
 *   window_size (B) = ws.
 * The tables are validated by the host (tacorl_amd/data/play_replay.py validate_play_tables) and every id they can produce
 * lies in [0, n_frames); idx, window, strategy (into [0, 1]), disp (>= 1), noise_step (into [-1, 1]), s, rs, the position
 * read in nn_val and the goal are nevertheless clamped into range before any table access or store, and *status is set to 1
 * (it is never cleared here) when such a clamp changed a value or an nn_val entry lay outside [0, n_frames).  All pointers are
 * device pointers, 8-byte (int64 / double) or 4-byte (float / int) aligned; nn_ptr / nn_val may be NULL when n_nn == 0,
 * noise_step may be NULL (no goal augmentation).  Nothing is allocated; a non-positive B, Tmax, A, n_items, n_episodes or
 * n_frames, n_nn < 0, min_window outside [1, Tmax], n_frames < Tmax, last_end outside [0, n_frames) or a NULL required /
 * misaligned pointer is refused with TACORL_EINVAL before anything is launched. */
int tacorl_sample_play_windows(const long* episode_lookup, long n_items, const long* ep_start, const long* ep_end,
                               int n_episodes, const long* nn_ptr, long n_nn, const long* nn_val, const float* actions,
                               long n_frames, long last_end, const long* idx, const long* window, const long* strategy,
                               const long* disp, const long* noise_step, const double* u_choice,
                               const double* u_random_state, int B, int Tmax, int A, int min_window, long* ids, float* act,
                               long* disp_out, long* window_size, int* status, tacorl_stream_t stream);
/* dst[r][0:cols] (+)= src[r % src_row_mod][0:cols]  (src_row_mod <= 0: r).  expand_obs on
 * embeddings instead of images (reference utils/misc.py:132-153) and torch.cat plumbing. */
int tacorl_copy_cols(const float* src, int ld_src, float* dst, int ld_dst, int rows, int cols,
                     int src_row_mod, int accumulate, tacorl_stream_t stream);
/* n <= 32 mutually independent tacorl_copy_cols in one launch (no copy may read what another writes). */
int tacorl_copy_cols_batch(int n, const float* const* src, const int* ld_src, float* const* dst,
                           const int* ld_dst, const int* rows, const int* cols,
                           const int* src_row_mod, const int* accumulate, tacorl_stream_t stream);
/* Vector observations (reference modules/cql/cql_offline_lightning_d4rl.py, modules/tacorl/tacorl_d4rl.py:68-89): the input
 * rows of the step's policy and Q chains in ONE launch, straight from the batch.  obs (B,T,S), goal (B,G), acts_main
 * ((3n+1) B, A) = [data action | uniform | n x pi(obs) | n x pi(next)], act_pi / act_next (B,A).  out[0..4] (any may be NULL):
 *   0: [B][lds] = [obs[b][0] | goal[b]]        1: [B][lds] = [obs[b][T-1] | goal[b]]
 *   2: [(3n+1) B][ldq] = [obs[r % B][0] | goal[r % B] | acts_main[r]]   (sample-major rows k B + b)
 *   3: [B][ldq] = [obs[b][0] | goal[b] | act_pi[b]]        4: [B][ldq] = [obs[b][T-1] | goal[b] | act_next[b]]
 * columns up to the leading dimension are written as zero.  out_bf16 (NULL, or five pointers of which any may be NULL):
 * bf16 mirrors of the same blocks at the same leading dimensions (round to nearest even).  lds >= S + G, ldq >= S + G + A,
 * both multiples of 4; fp32 outputs 16-byte, mirrors 8-byte aligned; a Q block needs its action pointer.  Grid-stride over
 * at most tacorl_vec_rows_max_blocks() workgroups of 256 threads (one thread per row and four columns). */
int tacorl_vec_rows_max_blocks(void);
int tacorl_vec_rows(const float* obs, const float* goal, const float* acts_main, const float* act_pi,
                    const float* act_next, float* const* out, void* const* out_bf16, int B, int T, int S, int G, int A,
                    int n, int lds, int ldq, tacorl_stream_t stream);
/* out[b][c] = sum_{j<reps} in[j*B+b][c] : gradient of that broadcast. */
int tacorl_reduce_rows_mod(const float* in, int ld_in, float* out, int ld_out, int B, int cols,
                           int reps, tacorl_stream_t stream);
/* n <= 4 such reductions of one shape in one launch. */
int tacorl_reduce_rows_mod_batch(int n, const float* const* in, int ld_in, float* const* out, int ld_out, int B,
                                 int cols, int reps, tacorl_stream_t stream);
/* dst[r][0:A] = 2u-1 (last dim snapped to +-1 for a discrete gripper);
 * reference modules/cql/cql_offline_lightning.py:243-250. */
int tacorl_uniform_actions(const float* u01, float* dst, int ld_dst, int rows, int A,
                           int discrete_gripper, tacorl_stream_t stream);

/* ---- tanh-Gaussian policy head (reference actor.py:65-156, utils/distributions.py:61-153) --- */
/* head[m] = [mean_raw(Ac) | log_std_raw(Ac) | gripper logits(2)?].  For k<n, m<M:
 * a = tanh(mu + sd*eps[k][m]) -> act_out[(k*M+m)*ld_act ..], log pi -> logp[k*M+m].
 * gumbel_u (n,M,2) U(0,1) or NULL: discrete gripper (hard_rsample: the rsample(hard=True) index). */
int tacorl_tanh_normal_sample(const float* head, int ld_head, const float* eps, const float* gumbel_u,
                              int hard_rsample, float* act_out, int ld_act, float* logp, int* grip_idx,
                              int n, int M, int Ac, tacorl_stream_t stream);
/* njobs <= 6 tacorl_tanh_normal_sample calls sharing (M, Ac, ld_head, ld_act) in one launch, optionally with
 * the tacorl_uniform_actions(u01, u_dst, ld_act, u_rows, A, u_discrete) of the step (u01 NULL = none). */
int tacorl_tanh_normal_sample_batch(int njobs, const float* const* head, int ld_head,
                                    const float* const* eps, const float* const* gumbel_u,
                                    const int* hard_rsample, float* const* act_out, int ld_act,
                                    float* const* logp, int* const* grip_idx, const int* n, int M, int Ac,
                                    const float* u01, float* u_dst, int u_rows, int A, int u_discrete,
                                    tacorl_stream_t stream);

/* ---- plan-recognition transformer glue (reference plan_recognition_transformer.py:70-105) ---- */
/* out[r] = [x[r] (D, zero-padded to Dp)] + add[r % T]  (position embeddings). */
int tacorl_add_rows_bcast(const float* x, int ldx, const float* add, float* out, int R, int T, int D,
                          int Dp, tacorl_stream_t stream);
/* softmax(q k^T / sqrt(hd)) v per (batch, head); qkv [B*T][3D], out [B*T][D]; T <= 64, hd <= 16. */
int tacorl_attention_fwd(const float* qkv, float* out, int B, int T, int D, int H, tacorl_stream_t stream);
/* Train mode of the same (reference plan_recognition_transformer.py:49-54: nn.TransformerEncoderLayer(dropout=p);
 * nn.MultiheadAttention drops attention probabilities): keep = uint8 [B][H][T][T] keep flags (an explicit input:
 * the caller draws them), kept probabilities are scaled by keep_scale = 1/(1-p). */
int tacorl_attention_dropout_fwd(const float* qkv, float* out, const unsigned char* keep, float keep_scale, int B,
                                 int T, int D, int H, tacorl_stream_t stream);
int tacorl_attention_dropout_bwd(const float* qkv, const float* d_out, float* d_qkv, const unsigned char* keep,
                                 float keep_scale, int B, int T, int D, int H, tacorl_stream_t stream);
/* nn.Dropout in train mode with an explicit keep mask, in place: x[i] = keep[i] ? x[i] * keep_scale : 0
 * (an activation in the forward, its gradient in the backward; :60,87 and the encoder layers' dropout1/2/ffn). */
int tacorl_dropout_mul(float* x, const unsigned char* keep, float keep_scale, long n, tacorl_stream_t stream);
/* y = LayerNorm(x + res); stats[r] = {mean, rstd} (may be NULL). D <= 256. */
int tacorl_add_layernorm_fwd(const float* x, const float* res, const float* w, const float* b, float* y,
                             float* stats, int R, int D, float eps, tacorl_stream_t stream);
/* Frozen / eval plan-recognition encoder in ONE launch: position embedding + L post-norm transformer
 * encoder layers (ReLU FFN) + mean over time -> pooled [B][D]; d_model 32 or 64 (one or two cameras), T 16 or 32, 8 heads,
 * FF % 256 == 0, L <= 4 (reference plan_recognition_transformer.py:36-88).  One workgroup per sequence, bf16 MFMA, nothing
 * saved for a backward.  offsets: [position_embeddings, then per layer in_proj_weight, in_proj_bias,
 * out_proj.weight, out_proj.bias, linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm1.weight,
 * norm1.bias, norm2.weight, norm2.bias] - element offsets into params and its bf16 copy params_bf16. */
int tacorl_pr_encoder_fused_supported(int D, int T, int H, int FF, int L);
/* the train-mode launches (tacorl_pr_encoder_fused_train / _train_sample) exist for d_model 32 (T 16 or 32); the one-launch
 * backward for T 16 */
int tacorl_pr_encoder_fused_train_supported(int D, int T, int H, int FF, int L);
int tacorl_pr_encoder_fused(const float* emb, int ld_emb, const float* params, const void* params_bf16,
                            const long* offsets, float* pooled, int B, int D, int T, int H, int FF, int L,
                            tacorl_stream_t stream);
/* The same launch extended by the posterior head and the plan sample: head = Wc pooled + bc with (Wc, bc) the
 * composition of the two bias-only Linear layers after the pooling (fc, mean_fc: no activation between them;
 * tacorl_pr_head_compose, weights only, off the dependent chain), std = softplus(var_raw) + min_std,
 * plan = tanh(mean + eps * std)  (plan_recognition_transformer.py:89-104).  2A <= 64. */
int tacorl_pr_encoder_fused_sample(const float* emb, int ld_emb, const float* params, const void* params_bf16,
                                   const long* offsets, float* pooled, int B, int D, int T, int H, int FF, int L,
                                   const float* Wc, const float* bc, const float* eps, float* head, float* plan,
                                   int A, float min_std, tacorl_stream_t stream);
/* tacorl_pr_encoder_fused_sample that also writes the action decoder's bf16 input rows behind each sequence's plan sample -
 * bit for bit what tacorl_build_ad_input_bf16(plan, emb_ad, ld_ad, xb_seq, B, T, Tm, P, E) writes in a launch of its own
 * behind this one: xb_seq[(t B + b)][0..127] = bf16([plan_b | emb_ad[b T + t][0..E) | 0 ...]) for t < Tm; rows t >= Tm are not
 * touched.  d_model 32; P == A, P % 8 == 0, P + E <= 128, 1 <= Tm <= T, ld_ad >= E, xb_seq 16-byte aligned - TACORL_EINVAL
 * otherwise, nothing launched. */
int tacorl_pr_encoder_fused_sample_rows(const float* emb, int ld_emb, const float* params, const void* params_bf16,
                                        const long* offsets, float* pooled, int B, int D, int T, int H, int FF, int L,
                                        const float* Wc, const float* bc, const float* eps, float* head, float* plan,
                                        int A, float min_std, void* xb_seq, int Tm, int P, int E, const float* emb_ad,
                                        int ld_ad, tacorl_stream_t stream);
/* Train mode of the same launch (PlayLMP.training_step with plan-recognition dropout 0): additionally writes, per layer, the
 * tensors the per-op backward reads, in the per-op forward's layouts (fp32, batch-major rows).  save[9 l + k], k = 0..8: layer
 * input [B T][32], q|k|v [B T][96], attention output [B T][32], out-projection [B T][32], LayerNorm-1 output [B T][32],
 * post-ReLU FFN hidden [B T][FF], FFN output [B T][32], LayerNorm-1 {mean, rstd} [B T][2], LayerNorm-2 {mean, rstd} [B T][2]. */
int tacorl_pr_encoder_fused_train(const float* emb, int ld_emb, const float* params, const void* params_bf16,
                                  const long* offsets, float* pooled, int B, int D, int T, int H, int FF, int L,
                                  float* const* save, tacorl_stream_t stream);
/* Train-mode backward of the same encoder: the input-gradient chain of all layers in ONE launch (+ one small reduce), from
 * d_pool [B][32] (gradient of the time-pooled output) to dx [B T][32] (gradient of the position-embedded input).
 * saved[9 l + k]: what tacorl_pr_encoder_fused_train wrote.  dz[4 l + k], k = 0..3, outputs - the dZ operands of the per-op
 * weight-gradient GEMMs: LayerNorm-2 input gradient [B T][32] (linear2), masked hidden gradient [B T][FF] (linear1),
 * LayerNorm-1 input gradient [B T][32] (out_proj), d(q|k|v) [B T][96] (in_proj).  wt[4 l + {0, 1, 2, 3}]: linear1.weight^T
 * [32][FF], linear2.weight^T [FF][32], out_proj.weight^T [32][32], in_proj_weight^T [32][96] as bf16
 * (tacorl_transpose_to_bf16; the last two may be NULL: gathered from the fp32 block inside the launch).  ln_part: scratch of L * 2 * B * 64 floats;
 * ln_grads[4 l + k]: norm1.weight, norm1.bias, norm2.weight, norm2.bias gradients (written, not accumulated).
 * d_pool == NULL: d_pool = d_head Wc computed in the launch (d_head [B][A2], Wc [A2][32] from tacorl_pr_head_compose).
 * Reference: autograd through plan_recognition_transformer.py:70-88 (nn.TransformerEncoderLayer, post-norm, ReLU). */
int tacorl_pr_encoder_bwd_fused(const float* params, const long* offsets, const float* d_pool, const float* d_head,
                                const float* Wc, int A2, float* dx, const float* const* saved, float* const* dz,
                                const void* const* wt, float* ln_part, float* const* ln_grads, int B, int D, int T, int H,
                                int FF, int L, tacorl_stream_t stream);
/* tacorl_pr_encoder_fused_train with the posterior head and the plan sample in the launch (head = Wc pooled + bc, composed
 * by tacorl_pr_head_compose; plan = tanh(mean + eps * std)); its backward: tacorl_pr_encoder_bwd_fused with d_pool == NULL. */
int tacorl_pr_encoder_fused_train_sample(const float* emb, int ld_emb, const float* params, const void* params_bf16,
                                         const long* offsets, float* pooled, int B, int D, int T, int H, int FF, int L,
                                         float* const* save, const float* Wc, const float* bc, const float* eps,
                                         float* head, float* plan, int A, float min_std, tacorl_stream_t stream);
int tacorl_pr_head_compose(const float* w_fc, const float* b_fc, const float* w_head, const float* b_head,
                           float* Wc, float* bc, int D, int FC, int A2, tacorl_stream_t stream);
int tacorl_mean_over_t(const float* x, float* out, int B, int T, int D, tacorl_stream_t stream);
/* head [B][2A] = [mean | var_raw]; std = softplus(var_raw)+min_std; plan = tanh(mean + eps*std). */
int tacorl_pr_sample(const float* head, const float* eps, float* plan, float* mu_out, float* std_out,
                     int B, int A, float min_std, tacorl_stream_t stream);

/* ---- action decoder (reference networks/action_decoders/action_decoder_logistic.py) ---------- */
/* Time-major RNN input x[(t*B+b)] = [plan[b] | emb[b*T+t]], t < Tm (:279-281). */
int tacorl_build_ad_input(const float* plan, const float* emb, int ld_emb, float* out, int B, int T,
                          int Tm, int P, int E, tacorl_stream_t stream);
/* bf16 compute: the RNN's layer-0 input projection straight from (plan, frame embeddings), without x_seq:
 * out[t*B + b][n] = b_ih[n] + sum_k bf16(x[k]) bf16(w_ih[n][k]), x = [plan[b] (P) | emb[b*T + t] (E)], P + E <= 64, H % 16 == 0
 * (reference action_decoder_logistic.py:279-281 + nn.RNN's weight_ih_l0). */
int tacorl_ad_input_proj(const float* plan, const float* emb, int ld_emb, const float* w_ih, const float* b_ih,
                         float* out, int B, int T, int Tm, int P, int E, int H, tacorl_stream_t stream);
size_t tacorl_logistic_mixture_ws_bytes(int B, int Tm, int Da);
/* Discretised-logistic-mixture NLL + gripper CE (:110-235), forward + backward fused.
 * heads[(t*B+b)] = [means Da*K | log_scales Da*K | logit_probs Da*K | gripper 2]; actions batch-major
 * [B][T][Da+1]; d_heads may be NULL (loss only); loss_out: two device floats {loss, gripper accuracy}. */
int tacorl_logistic_mixture_loss(const float* heads, int ldh, const float* actions, float* d_heads,
                                 float* loss_out, int B, int T, int Tm, int Da, int K, int num_classes,
                                 float gripper_alpha, float grad_scale, void* ws, size_t ws_bytes,
                                 tacorl_stream_t stream);
/* loss_out may be NULL: the per-block partial sums then stay in ws, and this call - any time before the next
 * tacorl_logistic_mixture_loss on the same ws, same (B, Tm, Da) - writes {loss, gripper accuracy} (a loss that is only
 * logged, reference tacorl.py:262-270, need not cost a launch per step). */
int tacorl_logistic_mixture_finish(const void* ws, size_t ws_bytes, int B, int Tm, int Da, float* loss_out,
                                   tacorl_stream_t stream);
/* ActionDecoderLogistic._sample (:238-266), the action of `act` at rollout time: Gumbel-max mixture component,
 * inversion sampling of the chosen logistic, argmax gripper class.  rand_a [R][Da][K], rand_b [R][Da]: the
 * caller's U(0,1) draws in the heads' row order; out [R][Da+1] = [actions | gripper -1/+1]. */
int tacorl_logistic_mixture_sample(const float* heads, int ldh, const float* rand_a, const float* rand_b,
                                   float* out, int R, int Da, int K, tacorl_stream_t stream);

/* The same three without the gripper head (discrete_gripper: False, :52,134-138,265-266 - the D4RL decoder): every action
 * dimension is a mixture dimension.  heads[(t*B+b)] = [means Da*K | log_scales Da*K | logit_probs Da*K], ldh >= 3*Da*K;
 * actions batch-major [B][T][Da]; no cross-entropy term; loss_out: two device floats {loss, 0}; the sample writes
 * out [R][Da].  ws: tacorl_logistic_mixture_ws_bytes(B, Tm, Da).  Always the 16-lane kernel (TACORL_LM_SCALAR is not read),
 * so a lazy loss (loss_out NULL) is finished by tacorl_logistic_mixture_nogrip_finish, not by the gripper variant's. */
int tacorl_logistic_mixture_nogrip_loss(const float* heads, int ldh, const float* actions, float* d_heads,
                                        float* loss_out, int B, int T, int Tm, int Da, int K, int num_classes,
                                        float grad_scale, void* ws, size_t ws_bytes, tacorl_stream_t stream);
int tacorl_logistic_mixture_nogrip_finish(const void* ws, size_t ws_bytes, int B, int Tm, int Da, float* loss_out,
                                          tacorl_stream_t stream);
int tacorl_logistic_mixture_nogrip_sample(const float* heads, int ldh, const float* rand_a, const float* rand_b,
                                          float* out, int R, int Da, int K, tacorl_stream_t stream);

/* ---- backward glue: ReLU-RNN BPTT, transformer, seq-VAE KL ---------------------------------- */
int tacorl_relu_mask_mul(const float* dy, const float* add, const float* h, float* out, long n,
                         tacorl_stream_t stream);
/* accumulate: 0 = overwrite rows t < Tm, 1 = add to them, 2 = overwrite them and zero the rows Tm <= t < T */
int tacorl_ad_input_bwd(const float* dx, float* d_plan, float* d_emb, int ld_emb, int B, int T, int Tm,
                        int P, int E, int accumulate, tacorl_stream_t stream);
/* PlayLMP.training_step (reference play_lmp_for_rl.py:200-257): the gradient entering the encoders in one launch.
 * d_emb [(b T + t)][Ec] (holding the action decoder's share) += dx[..][0..D_in) (plan recognition) + dS[b][0..Ec) on t = 0
 * (plan proposal, state) + dgin[b][0..Ec) on t = T - 1 (plan proposal, goal), in that order; camera j's 32 columns also go
 * to f_dout[j] [(b T + t)][32] (NULL: skipped).  Ec = 32 ncam. */
int tacorl_plmp_demb_finish(float* d_emb, const float* dx, int ld_dx, int D_in, const float* dS, int ld_ds,
                            const float* dgin, float* const* f_dout, int ncam, int B, int T, int Ec,
                            tacorl_stream_t stream);
int tacorl_bcast_over_t(const float* src, float* dst, int B, int T, int D, float scale, int accumulate,
                        tacorl_stream_t stream);
int tacorl_attention_bwd(const float* qkv, const float* d_out, float* d_qkv, int B, int T, int D, int H,
                         tacorl_stream_t stream);
size_t tacorl_add_layernorm_bwd_ws_bytes(int R, int D);
int tacorl_add_layernorm_bwd(const float* dy, const float* x, const float* res, const float* w,
                             const float* stats, float* dv, float* dw, float* db, int R, int D,
                             int accumulate, void* ws, size_t ws_bytes, tacorl_stream_t stream);
/* Balanced KL(q||p) of PlayLMP.compute_kl_loss (reference play_lmp_for_rl.py:259-301), fwd+bwd:
 * out2 = {kl, kl_beta*kl}; d_head_* = d(kl_beta*kl)/d(raw heads) * grad_scale. */
int tacorl_gauss_kl_balanced(const float* head_q, const float* head_p, float* d_head_q, float* d_head_p,
                             int B, int A, float kl_alpha, float kl_beta, float min_std, int balanced,
                             float grad_scale, float* out2, tacorl_stream_t stream);
int tacorl_pr_sample_bwd(const float* head, const float* eps, const float* d_plan, float* d_head, int B,
                         int A, float min_std, tacorl_stream_t stream);

/* device-resident metric record written by the loss kernels (names = reference self.log keys) */
enum {
  TACORL_LG_ALPHA_LOSS = 0, TACORL_LG_ALPHA, TACORL_LG_ACTOR_LOSS, TACORL_LG_BELL1, TACORL_LG_BELL2,
  TACORL_LG_CONS1, TACORL_LG_CONS2, TACORL_LG_Q1LOSS, TACORL_LG_Q2LOSS, TACORL_LG_ALPHA_P,
  TACORL_LG_ALPHA_P_LOSS, TACORL_LG_Q1_DATA, TACORL_LG_Q1_RAND, TACORL_LG_Q1_POL, TACORL_LG_Q2_DATA,
  TACORL_LG_Q2_RAND, TACORL_LG_Q2_POL, TACORL_LG_ACTION_LOSS,
  TACORL_LG_ACTION_ACC /* second float of the action decoder's loss output, not logged */, TACORL_LG_Q1_DR3, TACORL_LG_Q2_DR3,
  TACORL_LG_COUNT
};
/* alpha_loss and d/dlog_alpha (cql_offline_lightning.py:447-449); grad scaled by grad_scale. */
int tacorl_alpha_loss(const float* logp, int B, const float* log_alpha, float target_entropy,
                      float grad_scale, float* g_log_alpha, float* logs, tacorl_stream_t stream);
/* One GPU: the same loss / gradient and Adam's step on log_alpha in ONE launch (adam arithmetic of tacorl_adam_step for
 * n = 1 without clipping; the logged loss uses the pre-step log_alpha, reference cql_offline_lightning.py:447-455). */
int tacorl_alpha_loss_step(const float* logp, int B, float* log_alpha, float target_entropy, float* g_log_alpha,
                           float* logs, float* m, float* v, float lr, int* step_counter, tacorl_stream_t stream);
/* Q phase actor loss mean(alpha*logpi - min(q1,q2)) and dL/dq_i (:463-466). */
int tacorl_actor_qmin(const float* q1, const float* q2, const float* logp, int B, const float* log_alpha,
                      float* dq1, float* dq2, float grad_scale, float* logs, tacorl_stream_t stream);
/* dL_actor/d head.  g_act1/2: dL/da from the critics (Q phase) or NULL; value: dataset action for
 * the BC phase (:459-461) or NULL. */
int tacorl_actor_head_bwd(const float* head, int ld_head, const float* eps, const float* logp,
                          const float* g_act1, const float* g_act2, int ld_g, const float* value,
                          int ld_value, const int* grip_idx, const float* log_alpha, float grad_scale,
                          float* d_head, int B, int Ac, int has_grip, float* logs, tacorl_stream_t stream);
/* Behaviour-cloning loss of a policy head against a target (relay imitation learning): loss_out[0] = -mean_m
 * Actor.log_prob(target_m) (actor.py:140-156: target clamped to +-0.999, mean to +-9, log-std to [-5, 2], the gripper's
 * GumbelSoftmax.log_prob at has_grip) and d_head = grad_scale * d loss / d head ([M][ld_head], the columns of head), in one
 * launch.  head: [M][ld_head] = [mean (Ac) | log-std (Ac) | gripper logits (2)]; target: [M][ld_target] = [Ac values |
 * gripper +-1].  The per-element arithmetic is tacorl_actor_head_bwd's `value` term; the mean is a fixed-order sum. */
int tacorl_tanh_normal_nll(const float* head, int ld_head, const float* target, int ld_target, int M, int Ac,
                           int has_grip, float grad_scale, float* d_head, float* loss_out, tacorl_stream_t stream);

/* ---- DR3 regulariser of the critics (reference cql_offline_lightning.py:424-437, 496-499) ---------- */
/* For each of n <= 2 critics k, one workgroup each, in ONE launch: emb_obs[k], emb_next[k] are (B, Eo) fp32 rows with
 * leading dimensions ld_obs, ld_next (the critic's own encoder over the observation cameras; emb_next is a constant).
 *   v_k = coef / B * sum_b sum_j emb_obs[k][b][j] * emb_next[k][b][j]
 *   logs[dr3_slots[k]] = v_k;  logs[loss_slots[k]] += v_k
 *   d_obs[k][b][j] += coef * grad_scale / B * emb_next[k][b][j]   (rows of leading dimension ld_d; columns >= Eo untouched)
 * Fixed summation order, no atomics (bit-reproducible); fp32 arithmetic whatever the compute mode; no allocation.
 * TACORL_EINVAL before any launch for n outside 1..2, B < 1, Eo < 1, Eo % 32 != 0, a null pointer, a leading dimension
 * < Eo, a slot outside the record or two outputs that share a word. */
int tacorl_dr3_fwd_bwd(int n, const float* const* emb_obs, int ld_obs, const float* const* emb_next, int ld_next,
                       float* const* d_obs, int ld_d, int B, int Eo, float coef, float grad_scale, float* logs,
                       const int* dr3_slots, const int* loss_slots, tacorl_stream_t stream);

/* ---- Bellman + CQL logsumexp (+ Lagrange), forward and backward fused (:284-406) -------------- */
size_t tacorl_cql_ws_bytes(int B);
/* q_i / dq_i: rows [data B | random nB | current-policy nB | next-policy nB], sample-major (k*B+b). */
int tacorl_cql_loss(const float* q1, const float* q2, float* dq1, float* dq2, const float* tq1,
                    const float* tq2, const float* logp_cur, const float* logp_nxt, const float* next_logp,
                    const float* reward, const float* done, const float* log_alpha,
                    const float* log_alpha_prime, int B, int n, int A, float discount, float reward_scale,
                    float temp, float cons_w, float gap, int deterministic_backup, float grad_scale,
                    float* g_log_alpha_prime, float* logs, void* ws, size_t ws_bytes, tacorl_stream_t stream);

/* ---- clip_grad_norm_ + Adam + Polyak over one flat block (:229-232, 519-542, 553-574) --------- */
size_t tacorl_adam_ws_bytes(long n);
/* max_norm <= 0: no clipping; target NULL: no soft update; step_counter: device int (t-1). */
int tacorl_adam_step(float* param, const float* grad, float* m, float* v, long n, float lr,
                     float max_norm, int* step_counter, float* target, float tau, void* ws,
                     size_t ws_bytes, tacorl_stream_t stream);
/* nb <= 8 parameter blocks (each with its own lr / max_norm / step counter / optional Polyak target) in
 * two launches (norms + step counters, updates); results bit-identical to nb tacorl_adam_step calls
 * (checked by tests/test_heads_gpu.py test_adam_step_batch_mirror). */
size_t tacorl_adam_batch_ws_bytes(int nb);
int tacorl_adam_step_batch(int nb, float* const* param, const float* const* grad, float* const* m,
                           float* const* v, const long* n, const float* lr, const float* max_norm,
                           int* const* step_counter, float* const* target, const float* tau, void* ws,
                           size_t ws_bytes, tacorl_stream_t stream);
/* The same update; mirror[b] / target_mirror[b] (either array or any entry may be NULL): bf16 copies of the UPDATED
 * parameter block / Polyak target at the same element offsets, written by the update launch itself - the fused MLP
 * kernels' MFMA operand (params_bf16 of tacorl_mlp_fwd_fused) is then current when the step ends and the next step needs
 * no tacorl_to_bf16_batch launch at the head of its dependent chain. */
int tacorl_adam_step_batch_mirror(int nb, float* const* param, const float* const* grad, float* const* m,
                                  float* const* v, const long* n, const float* lr, const float* max_norm,
                                  int* const* step_counter, float* const* target, const float* tau,
                                  void* const* mirror, void* const* target_mirror, void* ws, size_t ws_bytes,
                                  tacorl_stream_t stream);

/* ---- evaluation: cross-entropy-method refinement ---------------------------------- */
/* CEMOptimizer.get_action (reference modules/cem/cem.py:69-104; evaluation/rollout_manager.py:99-136, :331-369) for R
 * independent problem rows in ONE launch, one workgroup per row: `iters` times { population = clamp(mean + std * eps, -1, 1)
 * (last dimension snapped to +-1 with discrete_gripper) -> Q of the N candidates -> the n_elite largest -> mean / std
 * blended with alpha towards the elites' mean / unbiased std, std clamped to [min_std, max_std] }; out[r] = the best elite of
 * all iterations (strict >).
 *   nnet = 1: Q = net 0 (what the reference executes: it evaluates q1 twice); nnet = 2: Q = min(net 0, net 1).
 *   s[n]: [R][E] embedding of the observation as net n's own encoders see it; params[n]: the net's Q head,
 *   tacorl_mlp_param_layout of [E + A, hidden x q_layers, 1] with SiLU hidden layers (16-byte aligned);
 *   params_bf16[n]: its bf16 mirror at the same element offsets (8-byte aligned; TACORL_BF16 only, else may be NULL).
 *   mean0: [R][A] or NULL (zeros); eps: [R][iters][N][A] standard-normal draws; out: [R][A].
 *   t_*: optional per-iteration trace (each may be NULL): population [R][iters][N][A], Q [R][iters][N], elite indices by
 *   descending Q [R][iters][n_elite], mean and std after the update [R][iters][A].
 *   ws: tacorl_cem_ws_bytes; on return [R][1 + 2 A] floats: best Q, final mean, final std of every row.
 * Supported: hidden = 256, N a multiple of 64 up to 256, A <= 32, E <= 256, 2 <= q_layers <= 4; 2 <= n_elite <= N.
 * TACORL_F32: fp32 MFMA on the fp32 weights; TACORL_BF16: bf16 MFMA on the mirror, activations rounded to bf16, fp32
 * accumulation.  Population, Q values, selection and statistics are fp32 in both.  Arguments are validated before
 * anything touches the device. */
int tacorl_cem_supported(int N, int A, int E, int hidden, int q_layers, int compute_dtype);
size_t tacorl_cem_ws_bytes(int R, int N, int A, int E, int hidden, int q_layers, int compute_dtype); /* 0: not supported */
int tacorl_cem_refine(int R, int nnet, const float* const* s, const float* const* params,
                      const void* const* params_bf16, const float* mean0, const float* eps, float* out, int N, int A,
                      int E, int hidden, int q_layers, int iters, int n_elite, float min_std, float max_std, float alpha,
                      int discrete_gripper, int compute_dtype, float* t_pop, float* t_q, int* t_elite, float* t_mean,
                      float* t_std, void* ws, size_t ws_bytes, tacorl_stream_t stream);

/* ---- neighbour table of the similar_robot_obs goal strategy (knn_ops.hip) ----
 * The exact brute-force L2 k-NN the reference builds with faiss.IndexFlatL2 (set_nn_steps_from_step,
 * datamodule/dataset/play_dataset.py:183-234, goal_cond_replay_buffer_dataset.py:76-130), stated so that it can be
 * reproduced bit for bit:
 *   points: (n_points, D) fp32 at a row pitch of ld floats (ld >= D: a column slice of a wider table is fine);
 *   d(q, p) in fp32, sequentially over j = 0 .. D-1: acc = acc + (q_j - p_j) * (q_j - p_j), every subtract, multiply and add
 *   rounded once (the direct form, no contraction; the expanded |q|^2 + |p|^2 - 2 q.p cancels on near-duplicate frames);
 *   the neighbours of query row q are the min(k, n_points) rows with the smallest (d, row), ascending - ties go to the lower
 *   row, the query's own row takes part and a duplicate at a lower row precedes it; absent entries (n_points < k) are row -1
 *   at distance +inf.
 * Queries are the rows [q0, q0 + n_queries) of the same table: a slice equals the same rows of the full run.
 *   nbr_row (n_queries, k) int32, nbr_dist (n_queries, k) fp32 or NULL; every element is written.
 * One thread per query, tacorl_knn_l2_query_block(k) queries per workgroup; the table streams through LDS in tiles of
 * tacorl_knn_l2_tile() rows; nothing of size n_points x n_points exists.  Deterministic.
 * Supported: 1 <= D <= 32, 1 <= k <= 64, n_points <= 2^31 - 1.  Device pointers, 4-byte aligned; nothing is allocated;
 * a NULL (but for nbr_dist) or misaligned pointer, ld < D, a query range outside the table, k or D out of range or a
 * non-positive size is refused with TACORL_EINVAL before anything is launched. */
int tacorl_knn_l2_supported(int D, int k);
int tacorl_knn_l2_tile(void);
int tacorl_knn_l2_query_block(int k); /* 0: k not supported */
int tacorl_knn_l2(const float* points, long n_points, int D, long ld, long q0, long n_queries, int k, int* nbr_row,
                  float* nbr_dist, tacorl_stream_t stream);
/* The reference's temporal filter, applied after the top-k as it does: with t = step_of_row[q0 + q] and s = step_of_row[r] for
 * each neighbour row r of query q in list order (rows outside [0, n_points), the absent entries, are skipped), s is dropped
 * iff s + margin > t > s - margin, i.e. |t - s| < margin (|t - s| == margin is kept; pure id arithmetic, it crosses episode
 * boundaries).  nn_steps (n_queries, k) int64: the surviving steps packed left in list order, -1 after; count (n_queries)
 * int32.  Every element of both is written.  step_of_row: (n_points) int64.  One thread per query.  A NULL or misaligned
 * pointer (8 bytes for the int64 tables), k outside 1..64, a query range outside the table, a negative margin or a
 * non-positive size is refused with TACORL_EINVAL before anything is launched. */
int tacorl_nn_margin_filter(const int* nbr_row, long n_queries, int k, long q0, const long* step_of_row, long n_points,
                            long margin, long* nn_steps, int* count, tacorl_stream_t stream);

/* ---- exact t-SNE of latent plans (tsne_ops.hip) ----
 * The embedding behind the reference's TSNEPlot callback (utils/callbacks/tsne_plot.py, "task_consistency").  The reference
 * calls MulticoreTSNE there: a Barnes-Hut approximation with a sparse 3 * perplexity-neighbour P and its own random
 * initialisation.  This is EXACT t-SNE with van der Maaten's optimiser constants and is not comparable with that library bit
 * for bit; as for tacorl_knn_l2 the yardstick is the fp64 restatement of THIS definition (tests/tsne_ref.py).
 *
 * Input.  X: (N, D) fp32 at a row pitch of ld floats (ld >= D), 1 <= D <= 32.  mean_c = (sum of column c) / N; M = the largest
 *   |x_rc - mean_c|; xn_rc = (x_rc - mean_c) / M, kept in ws as an (N, 32) table, zero beyond column D.  An all-equal table
 *   (M == 0) sets status[1] = 1 (the host refuses it; xn is then all zero and nothing faults).
 * Affinities.  d_ij = |xn_i - xn_j|^2 in the direct form of tacorl_knn_l2 (fp32, sequentially over the columns).  Per row i,
 *   with m_i = min_{j != i} d_ij and t_j = d_ij - m_i (the shift cancels in p): e_j = expf(-(beta_i t_j)), S = sum_{j != i} e_j,
 *   H_i = logf(S) + beta_i (sum_{j != i} e_j t_j) / S  - the entropy of p_{j|i} = e_j / S, p_{i|i} = 0.  beta_i is bisected: it
 *   starts at 1; while H_i > log(perplexity) it moves to the midpoint with the upper bracket, or doubles (capped at 1e30) while
 *   there is none; else to the midpoint with the lower bracket, or halves.  The search stops at the evaluation where
 *   |H_i - log(perplexity)| < 1e-5, or after 200 evaluations (the row is then counted in status[0]).
 *   P_ij = (p_{j|i} + p_{i|j}) / (2 N): dense (N, N) fp32, symmetric bit for bit, zero diagonal.  beta: (N), kept for inspection.
 *   Sums over j: lane l of the row's wave adds j = l, l + 64, ... in order, then a 6-step xor butterfly (32, 16, .. 1).
 * Forces.  For Y (N, 2), q_ij = |y_i - y_j|^2, w_ij = 1 / (1 + q_ij), w_ii = 0:
 *   attr_i = sum_j P_ij w_ij (y_i - y_j);  rep_i = sum_j w_ij^2 (y_i - y_j);  Z_i = sum_j w_ij;  Z = sum_i Z_i;
 *   grad_i = 4 (e attr_i - rep_i / Z) with exaggeration e.  Lane l of the row's wave adds j = 4 l + 256 k + {0, 1, 2, 3} in
 *   order, then the same butterfly: a row's three sums depend on that row of P and on Y only, and a run repeats bit for bit.
 * Update.  gains = gains + 0.2 where (grad > 0) != (u > 0), else gains * 0.8, floor 0.01;  u = momentum u - lr (gains grad);
 *   Y = Y + u;  then Y = Y - (column mean of Y).  Z and the two column sums are one tree each: thread t of 1024 adds the
 *   elements t, t + 1024, ... in order, then strides 512 .. 1 are folded in shared memory.
 * Schedule (the caller's: tacorl_amd/evaluation/tsne.py).  1000 iterations, lr 200; e = 12 and momentum 0.5 for the first 250,
 *   then e = 1 and momentum 0.8; Y0 = 1e-4 N(0, 1), u = 0, gains = 1.
 * Cost.  KL = sum_{P_ij > 0} P_ij log(P_ij / (w_ij / Z)), evaluated as sum P_ij (logf P_ij + logf(1 + q_ij)) + logf(Z) sum P_ij.
 *
 * Supported: 4 <= N <= tacorl_tsne_max_n() = 8192 (the dense P is N^2 * 4 B = 256 MiB there and is read once per iteration;
 * a row's distances take N * 4 B of LDS, four rows per workgroup), 1 <= D <= 32, 1 <= perplexity and 3 perplexity <= N - 1.
 * Nothing is allocated: ws holds tacorl_tsne_workspace_bytes(N) bytes, 16-byte aligned, and is shared by the three calls;
 * tacorl_tsne_workspace_offsets writes the byte offsets of {xn (N, 32), attr (N, 2), rep (N, 2), Z_i (N)} - what the last
 * tacorl_tsne_affinities / tacorl_tsne_step left there.  status: int[2].  Device pointers; P 16-byte, Y 8-byte, the others
 * 4-byte aligned.  A NULL or misaligned pointer, a short workspace, ld < D or a size, D or perplexity out of range is refused
 * with TACORL_EINVAL before anything is launched.  Asynchronous on `stream`; no atomics but the integer count in status[0]. */
int tacorl_tsne_supported(long N, int D);
int tacorl_tsne_max_n(void);
size_t tacorl_tsne_workspace_bytes(long N); /* 0: N not supported */
int tacorl_tsne_workspace_offsets(long N, long* off4);
int tacorl_tsne_affinities(const float* X, long N, int D, long ld, float perplexity, float* P, float* beta, int* status,
                           void* ws, size_t ws_bytes, tacorl_stream_t stream);
/* One iteration in place on Y, u, gains (each (N, 2)). */
int tacorl_tsne_step(const float* P, long N, float* Y, float* u, float* gains, float exaggeration, float momentum, float lr,
                     void* ws, size_t ws_bytes, tacorl_stream_t stream);
int tacorl_tsne_kl(const float* P, const float* Y, long N, float* out, void* ws, size_t ws_bytes, tacorl_stream_t stream);

/* ---- neighbour-sparse t-SNE of latent plans (tsne_ops.hip) ----
 * The same embedding above the dense path's 8192 rows: the reference library's sparse P over the K = floor(3 perplexity)
 * nearest neighbours (the product 3 perplexity in fp32), with the repulsion taken exactly over all pairs - Barnes-Hut at
 * theta = 0.  Nothing of size N x N exists.  Everything not stated here is the dense definition above, by the same kernels:
 * the input normalisation to xn, w_ij, the update, the centring, the schedule.  fp64 restatement: tests/tsne_nbr_ref.py.
 *
 * Neighbour lists.  N(i): the K rows j != i with the smallest (d_ij, j), ascending; d_ij in the direct form of tacorl_knn_l2
 *   on xn.  The row itself is left out by index, not by distance: a duplicate of row i is a neighbour at d = 0; ties go to
 *   the lower row.  nbr_row (N, K) int32, nbr_dist (N, K) fp32, every element written (K <= N - 1: no list has an absent
 *   entry).  A NaN distance counts as +inf (+inf itself, an overflow, is a distance like any other): a table with non-finite
 *   values still gives every row K valid rows - for a row whose distances are all NaN the K lowest other rows, at +inf - so
 *   nothing downstream addresses memory by a bad index; the conditionals of such a row are NaN and the row is counted in
 *   status[0].  tacorl_tsne_nbr_knn is that step alone on any (N, D) table at a row pitch of ld floats: one thread per query,
 *   64 queries per workgroup, the table through LDS in tiles of tacorl_tsne_nbr_knn_tile() rows, the lists (up to 96 KiB) in LDS.
 * Conditionals.  The dense bisection (start 1, tolerance 1e-5, 200 evaluations, capped rows counted in status[0]) over the K
 *   listed distances: m_i = the first neighbour's distance, t_s = d_s - m_i, e_s = expf(-(beta_i t_s)), S = sum_s e_s,
 *   H_i = logf(S) + beta_i (sum_s e_s t_s) / S; cond (N, K) fp32 = e_s / S in list order, beta (N) kept.  Sums over the list:
 *   lane l of the row's wave adds the positions l, l + 64, l + 128 in order, then the xor butterfly 32 .. 1.
 * Symmetric P as CSR.  Row i holds every column j with j in N(i) or i in N(j), ascending in j; the value is (a + b) / (2 N)
 *   with a = p_{j|i} if j in N(i), else 0, and b = p_{i|j} if i in N(j), else 0 - one fp32 addition and one division by
 *   2.f * (float)N, as the dense symmetrisation - so P is symmetric bit for bit.  row_ptr (N + 1) int32, col and val with the
 *   caller's capacity >= 2 N K entries (a hub row's in-degree is unbounded, the total is not); row_ptr[N] stays on the
 *   device.  A row's length is counted and its one-sided in-entries are appended with integer atomics, then every row is
 *   sorted by column: the result does not depend on the order in which the atomics landed.
 * Forces.  attr_i = sum over row i's stored entries e of P_e w (y_i - y_col(e)): lane l of the row's wave adds the entries
 *   l, l + 64, ... of the row in order, then the butterfly.  rep_i = sum_{j != i} w_ij^2 (y_i - y_j) and Z_i = sum_{j != i} w_ij
 *   over ALL j: the j range is cut into segments of L = tacorl_tsne_nbr_segment(N) = 256 ceil(N / 8192) rows (at most 32 of
 *   them); one thread adds a segment's j in ascending order from 0 (Y streams through LDS in tiles of 256), and the segments'
 *   partial sums are added in ascending segment order from 0.  No float atomics; a run repeats bit for bit.  Z and the update
 *   are the dense ones.  The grid is ceil(N / 256) x ceil(N / L) workgroups: 1024 at N = 8192, 16384 at N = 131072.
 * Cost.  Over the stored entries, in attr's order: sum P_e (logf P_e + logf(1 + q_e)) + logf(Z) sum P_e, Z as above.
 * Cross-check.  With K = N - 1 every list is the whole table, P has every off-diagonal entry, and this is, in real
 *   arithmetic, the dense definition (the entropy runs over the same N - 1 distances, m_i is their minimum); the two differ
 *   by the order of their sums only.
 *
 * Supported: 4 <= N <= tacorl_tsne_nbr_max_n() = 131072, 1 <= D <= 32, perplexity >= 1, K <= N - 1 and
 * K <= tacorl_tsne_nbr_max_k() = 192 (perplexity 40: K = 120).  Nothing is allocated: ws holds
 * tacorl_tsne_nbr_workspace_bytes(N) bytes, 16-byte aligned, shared by the three calls (about 66 MiB at N = 131072: xn and the
 * segments' partials); tacorl_tsne_nbr_workspace_offsets writes the byte offsets of {xn (N, 32), attr (N, 2), rep (N, 2),
 * Z_i (N)}.  status: int[2] as above.  Device pointers; Y 8-byte, ws 16-byte, the others 4-byte aligned.  A NULL or misaligned
 * pointer, a short workspace or capacity, ld < D or a size, D, K or perplexity out of range is refused with TACORL_EINVAL
 * before anything is launched.  Asynchronous on `stream`. */
int tacorl_tsne_nbr_supported(long N, int D, int K);
int tacorl_tsne_nbr_max_n(void);
int tacorl_tsne_nbr_max_k(void);
int tacorl_tsne_nbr_knn_tile(void);
int tacorl_tsne_nbr_segment(long N); /* 0: N not supported */
size_t tacorl_tsne_nbr_workspace_bytes(long N); /* 0: N not supported */
int tacorl_tsne_nbr_workspace_offsets(long N, long* off4);
int tacorl_tsne_nbr_knn(const float* points, long N, int D, long ld, int K, int* nbr_row, float* nbr_dist,
                        tacorl_stream_t stream);
int tacorl_tsne_nbr_affinities(const float* X, long N, int D, long ld, float perplexity, int* nbr_row, float* nbr_dist,
                               float* cond, float* beta, int* row_ptr, int* col, float* val, long capacity, int* status,
                               void* ws, size_t ws_bytes, tacorl_stream_t stream);
/* One iteration in place on Y, u, gains (each (N, 2)). */
int tacorl_tsne_nbr_step(const int* row_ptr, const int* col, const float* val, long N, float* Y, float* u, float* gains,
                         float exaggeration, float momentum, float lr, void* ws, size_t ws_bytes, tacorl_stream_t stream);
int tacorl_tsne_nbr_kl(const int* row_ptr, const int* col, const float* val, const float* Y, long N, float* out, void* ws,
                       size_t ws_bytes, tacorl_stream_t stream);

/* ---- rollout (rollout_ops.hip) ------------------------------------------------------ */
/* A linear layer with two inputs for a handful of rows, read from torch's row-major (N, K) fp32 masters as they lie:
 *   y[r][n] = act(b1[n] + b2[n] + sum_k w1[n][k] x1[r][k] + sum_k w2[n][k] x2[r][k]),   r < R, n < N.
 * One call is a ReLU-RNN cell of the action decoder's one-step rollout (reference action_decoder_logistic.py:87-97 through
 * nn.RNN: x1 the layer's input, x2 = h_{t-1}, act = RELU); with x2 == NULL (w2 and the flags are then ignored, b2 may still
 * be given) it is a head projection.  Where x2_row_is_zero[r] != 0 (R bytes, or NULL) row r of x2 counts as zeros and is
 * NOT READ: a plan that starts at this step has h_0 = 0 whatever the buffer holds (NaN included).
 * fp32 FMA throughout; a batched GEMV (one wave per neuron, tacorl_rows_linear2_group() rows of [x1 | x2] staged in LDS per
 * workgroup), each weight read once per row group.  Row determinism: y[r][n] depends on row r's inputs, its flag, n, K1, K2
 * and the weight pointers only - it is bit-identical whatever R is and wherever the row sits.
 * Shapes: 1 <= R <= 64, K1 >= 1, K2 >= 0, N >= 1 (each at most 2^24); K1, K2 and the leading dimensions need no alignment
 * beyond that of a float.  Shapes outside these, a NULL x1 / w1 / b1 / y (or w2 with x2 given and K2 > 0), ldx < K, ldy < N, a
 * misaligned pointer or y overlapping x1 or x2 is refused with TACORL_EINVAL before anything is launched. */
int tacorl_rows_linear2_supported(int R, int K1, int K2, int N);
int tacorl_rows_linear2_group(void);
int tacorl_rows_linear2_fwd(const float* x1, int ldx1, int K1, const float* w1, const float* b1, const float* x2, int ldx2,
                            int K2, const float* w2, const float* b2, const unsigned char* x2_row_is_zero, float* y, int ldy,
                            int R, int N, int act, tacorl_stream_t stream);

/* A whole MLP chain for a handful of rows (1 <= R <= 64) in ONE host call and without an allocation: n_layers (1..8) linear
 * layers dims[0] -> dims[1] -> .. -> dims[n_layers] with activations acts[l], weights w[l] (dims[l+1], dims[l]) row-major fp32
 * and biases b[l] as they lie in torch's masters (dims, w, b, acts: host arrays).  Every layer but the last is one launch of
 * the tacorl_rows_linear2_fwd kernel (x2 absent) on the caller's stream, so the per-neuron summation order and the row
 * determinism are that entry point's; there is no synchronisation between workgroups, layers are separate launches.
 * ws: the outputs of the layers before the last, layer l's (R, dims[l+1]) dense at offset R * (dims[1] + .. + dims[l]) - for
 * equal hidden widths (n_layers - 1) x R x hidden floats; they stay there after the call.  May be NULL with one layer.
 * The last layer, by mode:
 *   TACORL_ROWS_MLP_PLAIN          y (R, dims[n_layers]) = acts[last](..), an ordinary layer (a goal encoder);
 *   TACORL_ROWS_MLP_POLICY_ACTION  the layer is a policy head [fc_mean (Ac) | fc_log_std (Ac) | gripper_action (2)]
 *     (reference actor.py:65-104 with deterministic=True): y (R, Ac + dg) = [tanh(clamp(mean, -9, 9)) | gripper], the gripper
 *     column +1 where logit 1 > logit 0 and -1 otherwise (a tie is -1, torch.argmax's index 0).  Only the Ac mean rows and,
 *     with discrete_gripper, the two logit rows of the head are read; acts[last] is not applied.
 * npw: neurons per wave of the hidden layers, 1 or 2 (bit-identical results), 0 = the library's choice.
 * Refused with TACORL_EINVAL before anything is launched: R outside 1..64, n_layers outside 1..8, a width outside 1..2^24, a
 * NULL or misaligned (4 bytes) pointer, ldx < dims[0], ldy below the output width, an unknown mode / activation / npw, Ac < 1,
 * a head narrower than 2 Ac (+ 2 with discrete_gripper), y or ws overlapping x, a weight, a bias or each other. */
#define TACORL_ROWS_MLP_PLAIN 0
#define TACORL_ROWS_MLP_POLICY_ACTION 1
int tacorl_rows_mlp_supported(int R, int n_layers, const int* dims, int mode, int Ac, int discrete_gripper);
int tacorl_rows_mlp_npw(int N, int R); /* the neurons per wave npw = 0 stands for in a layer of N neurons and R rows */
int tacorl_rows_mlp_fwd(const float* x, int ldx, int n_layers, const int* dims, const float* const* w, const float* const* b,
                        const int* acts, float* ws, float* y, int ldy, int R, int mode, int Ac, int discrete_gripper, int npw,
                        tacorl_stream_t stream);

/* ---- a step's noise from a counter-based generator (DESIGN.md "Device noise"; tacorl_amd/noise.py restates it in NumPy) ----
 * Replaces the torch generator launches in front of a step (normal_ / uniform_ / bernoulli_): every element is a pure function
 * of (seed, step, draw id, global sample index, position inside the sample), computed by ONE launch for all of a step's buffers.
 * Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (j >> 2, sample0 + b, draw_id << 16 | k, step) for element j of
 * the `inner` elements of sample b, outer index k; element j takes output word j & 3 (a ragged last group leaves words unused).
 *   uniform: (w >> 8) 2^-24 in [0, 1);    keep: uniform < keep_p (uint8 1 / 0);
 *   normal:  Box-Muller on the word pairs (0,1) and (2,3): r = sqrt(-2 ln(((wa >> 8) + 1) 2^-24)), angle 2 pi (wb >> 8) 2^-24,
 *            outputs r cos, r sin in that order (accurate logf / sqrtf, sincospif on the exact argument 2 u2).
 * A segment is one destination buffer: n_outer x B_local x inner elements at `offset` (floats from base_f32; bytes from
 * base_u8 for a keep mask), laid out (B_local, n_outer, inner) or, with outer_major, (n_outer, B_local, inner).  One thread per
 * group of four; group0 = number of groups (n_outer B_local ceil(inner / 4)) of the segments in front.  Elements between
 * segments (alignment padding) are not written.
 * `segs` is a HOST table (tacorl_noise_table with n_seg rows, like the library's pointer arrays): it is checked on the host and
 * travels to the kernel as a launch argument, so the call stays asynchronous and a bad table is refused before anything is
 * launched.  Refused with TACORL_EINVAL: n_seg outside 1..TACORL_NOISE_MAX_SEGS, an unknown kind, draw_id or n_outer outside
 * 16 bits (n_outer >= 1), B_local / inner < 1, a segment that ends past n_f32 / n_u8 (the buffers' sizes in elements), keep_p
 * outside [0, 1], group0 / n_groups that are not the prefix sums, sample0 < 0, base_f32 not 16-byte aligned, a NULL base that
 * a segment needs. */
#define TACORL_NOISE_MAX_SEGS 64
enum { TACORL_NOISE_NORMAL = 0, TACORL_NOISE_UNIFORM = 1, TACORL_NOISE_KEEP = 2 };
typedef struct {
  int offset, kind, draw_id, n_outer, B_local, inner, outer_major;
  float keep_p;
  int group0, reserved;
} tacorl_noise_seg;
typedef struct {
  int n_f32, n_u8, n_groups, reserved;
  tacorl_noise_seg seg[1]; /* n_seg rows */
} tacorl_noise_table;
int tacorl_noise_fill(const void* segs, int n_seg, void* base_f32, void* base_u8, unsigned long long seed, unsigned int step,
                      int sample0, tacorl_stream_t stream);

/* ---- a rollout step's draws: the same generator, the sample and step words of the counter taken from a per-row table ----
 * Row r of a batch of up to TACORL_NOISE_ROWS_MAX environments runs its own episode at its own step, so
 *     counter = (j >> 2, episode[r], draw_id << 16, number[r])        key = (seed & 0xffffffff, seed >> 32)
 * with number[r] = step[r] (seg.which == 0) or plan_no[r] (seg.which == 1); the conversions are tacorl_noise_fill's (uniform,
 * normal).  An element is a function of (seed, draw id, episode, number, j) alone: not of the row, not of n_rows.  A segment
 * is (n_rows, inner) floats row-major at `offset` of base_f32; rows whose bit of `mask` is clear are NOT WRITTEN (and cost no
 * thread): the plan and CEM draws are needed for the rows that re-plan only.  One thread per group of four of the rows in the
 * mask, one launch for up to TACORL_NOISE_ROWS_SEGS segments.
 * `rows` is a HOST struct: checked on the host, then passed to the kernel BY VALUE in its launch arguments, so the call is
 * asynchronous, copies nothing and the caller may overwrite the struct as soon as the call returns.  Refused with
 * TACORL_EINVAL before anything is launched: n_rows outside 1..TACORL_NOISE_ROWS_MAX, n_seg outside
 * 1..TACORL_NOISE_ROWS_SEGS, a kind other than normal / uniform, which other than 0 / 1, draw_id outside 16 bits, inner < 1,
 * offset < 0 or a segment that ends past n_f32 (offset + n_rows inner), mask bits at or above n_rows, a non-zero reserved
 * field, base_f32 NULL or not 16-byte aligned.  A call whose masks are all empty launches nothing. */
#define TACORL_NOISE_ROWS_MAX 64
#define TACORL_NOISE_ROWS_SEGS 4
typedef struct {
  int offset, kind, draw_id, inner, which, reserved;
  unsigned long long mask;
} tacorl_noise_rows_seg;
typedef struct {
  int n_rows, n_seg, n_f32, reserved;
  unsigned int episode[TACORL_NOISE_ROWS_MAX], step[TACORL_NOISE_ROWS_MAX], plan_no[TACORL_NOISE_ROWS_MAX];
  tacorl_noise_rows_seg seg[TACORL_NOISE_ROWS_SEGS];
} tacorl_noise_rows;
int tacorl_noise_fill_rows(const void* rows, void* base_f32, unsigned long long seed, tacorl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

/* dcase_sed.h - C-ABI of libdcase_sed_mi355.so (gfx950 / MI355X).
 *
 * Drop-in boundary for ONE hot path of turpaultn/DCASE2019_task4: the mean-teacher CRNN train
 * step and its feature front-end.  The reference has no native code and no FFI;
 * what a maintainer binds these entry points to is the Python call sites listed next to each
 * declaration (paths relative to the reference root, baseline/...).  The Python host side that
 * mirrors those call sites lives in dcase2019_task4_amd/ and calls this library through ctypes
 * (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - plain C types, raw DEVICE pointers, explicit hipStream_t (passed as void*); no torch types.
 *  - the caller owns ALL memory (outputs, saved context, workspace).  The compute entry points never
 *    allocate, free or synchronise, so every one of them is hipGraph-capturable.  ONE family is the stated
 *    exception: the set-up calls of the data-parallel collective (sed_p2p_alloc / _configure / _open / _close /
 *    _free / _errors, below) allocate or map fine-grained device memory - which torch's allocator can neither
 *    create nor export - and synchronise the device; they run at construction / health-check time, never inside
 *    a step.  sed_p2p_allreduce itself follows the rule (one capturable launch).
 *  - return 0 on success, negative sed_status on failure; sed_last_error() gives a
 *    thread-local message.  Entry points are stateless and re-entrant.
 *  - activations are channels-last fp32: [B][T][F][C]; parameters keep the reference's
 *    shapes, packed into ONE flat fp32 buffer in named_parameters() order (sed_param_layout).
 */
#ifndef DCASE_SED_H
#define DCASE_SED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SED_OK = 0,
    SED_ERR_BAD_ARG = -1,        /* unsupported dims / null pointer */
    SED_ERR_WORKSPACE = -2,      /* ctx / workspace too small */
    SED_ERR_LAUNCH = -3,         /* HIP launch / runtime error */
    SED_ERR_UNSUPPORTED = -4     /* configuration outside the hot path */
} sed_status;

/* Model + batch geometry.  Mirrors the CRNN / CNN constructor arguments (baseline/models/CRNN.py:12-16,
 * CNN.py:35-38) on the hot path: activation="glu", attention=True, BGRU, 3 conv blocks with equal filter counts,
 * kernel 3 / stride 1 / pad 1, pooling (2,4) x3 (so F must be 64), n_in_channel = 1.
 *   C = 64,  H = 64,  SED_DTYPE_F32   cfg.crnn_kwargs (baseline/config.py:53-58): the specialised kernel set
 *   C in {64, 128}, H in {64, 256}, either dtype: the generic kernel set (gen.h) - BASELINE.json configs[4]'s wide CRNN
 *   (nb_filters 3 x 128, n_RNN_cell 256) and the bf16-operand variants of configs[2] / [4].
 * dtype selects the arithmetic (and, for bf16, the activation storage) of the step.  What runs on which operands, per mode:
 *   SED_DTYPE_F32     fp32 MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32: exact fp32 products, fp32 accumulation) in every
 *                     GEMM-shaped operator, fp32 storage - with ONE stated exception: conv block 0's backward forms its
 *                     conv0 / BatchNorm0 / GLU0 gradient sums D = P^T dlin, E = P^T dzgate on the bf16 MFMA with every fp32
 *                     operand split as hi + lo (two bf16) and three products hi hi + hi lo + lo hi (the lo lo term,
 *                     <= 2^-16 relative, is dropped), fp32 accumulation (csrc/blk0.hip).  Those gradients
 *                     (conv0.weight / bias, batchnorm0.weight / bias, glu0.linear.*) are asserted within 2e-4 of their
 *                     typical magnitude against the fp32 oracle (tests/test_gpu_parity.py; measured 1 - 3e-5), all others
 *                     at 1e-3 (measured ~1e-5).  Posteriors: <= 2e-5.
 *   SED_DTYPE_BF16    the fastest mode: operands rounded to bf16 (round-to-nearest-even), fp32 accumulation, AND bf16
 *                     storage of the conv-block activations.  bf16 operands: 3x3 convolutions forward / dgrad / wgrad, the
 *                     GLU's Linear forward / backward, conv block 0 forward and backward (single bf16 products), the GRU
 *                     weight-gradient GEMMs, and at H = 256 the W_hh / h operands of the recurrence and the gi / dX
 *                     projections.  fp32: the H = 64 recurrence, gates, heads, BatchNorm statistics, losses, Adam / EMA.
 *                     Measured posterior error against the fp32 oracle: 9.5e-4 (base geometry, B = 24), 1.25e-3 (base,
 *                     B = 64), 2.3e-3 (wide) - ABOVE the 1e-3 the north star names on two of three; tests assert the
 *                     measured bound + head-room and a 50-step loss trajectory.
 *   SED_DTYPE_BF16X3  split operands: every fp32 operand a is carried as a_hi + a_lo (both bf16) and a product is formed
 *                     as a_hi b_hi + a_hi b_lo + a_lo b_hi on the bf16 MFMA with fp32 accumulation - three MFMAs per
 *                     K = 16 (96 cycles against 512 for the exact-fp32 MFMA), relative error ~2^-16 per product; fp32
 *                     storage.  The conv-block GEMMs run this way (see DESIGN.md 3.11 for the list); everything else is as
 *                     in SED_DTYPE_F32.  This is the reduced-precision mode that HOLDS the north star's 1e-3 (asserted at
 *                     1e-3 on posteriors / 1e-2 on gradients, 11 geometries incl. the wide model).
 *   SED_DTYPE_F16     (round 5) the bf16 mode with its FORWARD chain in fp16: the operands of every forward GEMM-shaped
 *                     operator (conv block 0, the 3x3 convolutions, the GLU's Linear; at H = 256 the gi projections and the
 *                     W_hh / h operands of the recurrence) are rounded to fp16 (11-bit significand against bf16's 8; same
 *                     MFMA rate, same bytes) and the conv-block activations the forward hands on (p0, y1, p1, y2) are stored
 *                     as fp16.  Every forward tensor here is O(1) behind a BatchNorm: fp16's range (6e-5 .. 65504) covers
 *                     them, which it would NOT do for the gradients - so the BACKWARD is SED_DTYPE_BF16's, unchanged: the
 *                     forward kernels also write the bf16 copies of p0 / y1 / p1 / y2 that the backward kernels read, and
 *                     every gradient tensor and backward operand is bf16.  Why: the bf16 mode's posterior error has no
 *                     owner - every rounding site contributes 2.5 - 4e-4 and they add in quadrature
 *                     (profiles/r05_bf16_error_budget.md) - so no subset of operators can be promoted to reach 1e-3; eight
 *                     times less rounding error at every site can.  Posteriors are asserted at 1e-3 (measured: DESIGN.md 4c).
 *                     fp16 stores saturate at +-65504 (never Inf).
 * BatchNorm statistics, gates, the H = 64 recurrence, heads, losses and the optimiser are fp32 (fp64 sums) in all modes.
 * The mode is never chosen silently: the caller states it here. */
#define SED_DTYPE_F32 0
#define SED_DTYPE_BF16 1
#define SED_DTYPE_BF16X3 2
#define SED_DTYPE_F16 3
typedef struct {
    int32_t B;            /* clips in the batch                                  */
    int32_t T;            /* input frames (628 for BASELINE, 864 for config.py)  */
    int32_t F;            /* mel bins; must be 64                                */
    int32_t C;            /* conv filters per block: 64 or 128                   */
    int32_t H;            /* n_RNN_cell: 64 or 256                               */
    int32_t nclass;       /* <= 16 (10 in the reference)                         */
    int32_t n_layers_rnn; /* 1 or 2                                              */
    float   p_drop;       /* dropout probability (config.py:56), 0 disables      */
    float   bn_eps;       /* 1e-3 (models/CNN.py:49)                             */
    float   bn_momentum;  /* 0.99 (models/CNN.py:49)                             */
    int32_t dtype;        /* SED_DTYPE_F32 / SED_DTYPE_BF16 / SED_DTYPE_BF16X3 / SED_DTYPE_F16 */
} sed_dims;

/* Per-step scalars kept in DEVICE memory so that a captured hipGraph can be replayed while the
 * step counter, consistency weight, EMA alpha, Adam bias corrections and dropout seeds advance.
 * Restates the host arithmetic of main.train (main.py:72-78,127,155-157), ramps.sigmoid_rampup
 * (utils/ramps.py:20-27), update_ema_variables' alpha (main.py:47) and torch.optim.Adam's bias
 * correction.  Advanced by sed_step_state_advance(). */
typedef struct {
    int64_t  global_step;     /* main.py global_step BEFORE this step's increment       */
    int64_t  opt_step;        /* Adam step count of this step (1-based)                 */
    int64_t  rampup_length;   /* len(train_loader) * n_epoch // 2 (main.py:72)          */
    uint64_t base_seed;       /* user seed for the dropout / noise streams              */
    uint64_t seed_student;    /* Philox key for the student forward of this step        */
    uint64_t seed_teacher;    /* Philox key for the teacher forward of this step        */
    double   lr, beta1, beta2, eps;   /* torch.optim.Adam hyper-parameters (main.py:289) */
    double   ema_decay;       /* 0.999 (main.py:157)                                    */
    double   max_cons_cost;   /* cfg.max_consistency_cost = 2 (config.py:36)            */
    /* derived for this step: */
    float    cons_weight;     /* max_consistency_cost * rampup (main.py:74-78,127)      */
    float    ema_alpha;       /* min(1 - 1/(global_step+2), ema_decay) (main.py:47,155) */
    float    adam_step_size;  /* lr / (1 - beta1^opt_step)                              */
    float    adam_sqrt_bc2;   /* sqrt(1 - beta2^opt_step)                               */
} sed_step_state;

const char* sed_last_error(void);
int sed_version(void);

/* ---- parameter layout --------------------------------------------------------------------
 * Number of parameter tensors and their element offsets inside the flat buffer, in the
 * reference's named_parameters() order (cnn(18) -> rnn(8*n_layers) -> dense(2) ->
 * dense_softmax(2); models/CRNN.py:12-31).  offsets must hold n+1 entries (last = total). */
int sed_param_count(const sed_dims* d);
int sed_param_layout(const sed_dims* d, int64_t* offsets);

/* ---- CRNN forward / backward ---------------------------------------------------------------
 * Replaces CRNN.forward (models/CRNN.py:59-84) + CNN.forward (models/CNN.py:85-89) +
 * GLU.forward (CNN.py:11-16) + BidirectionalGRU.forward (RNN.py:14-16), called from
 * main.train (main.py:87,91) and evaluation (evaluation_measures.py:40-45,203-209).
 *   params      flat parameters (sed_param_layout)
 *   bn_running  [3][2][C] running_mean / running_var per block (read in eval; updated in train
 *               when update_bn != 0: BatchNorm2d momentum rule, CNN.py:49)
 *   bn_tracked  [3] int64 num_batches_tracked (incremented with bn_running), may be NULL
 *   x           [B][1][T][F] fp32
 *   train       1 = module.train() semantics (batch statistics, dropout), 0 = eval; | 4 = this batch's patch moments are
 *               already in ctx (sed_crnn_moments, below); 3 = train semantics for a forward whose
 *               backward will never run (the teacher's, main.py:87-89): bit 1 lets the library skip what only a backward reads
 *               (today: the bf16 activation copies of SED_DTYPE_F16); results are identical to train = 1
 *   seed_dev    device pointer to the 64-bit Philox key of this forward (ignored if p_drop==0
 *               or train==0); the same pointer/value must be given to backward
 *   ctx         saved activations for backward + scratch; sed_crnn_ctx_bytes(d)
 *   strong/weak outputs [B][T/8][nclass], [B][nclass].  train == 1 only: BOTH may be NULL - the output heads
 *               (models/CRNN.py:74-81) are then left to a sed_mt_step_backward call on the same ctx           */
size_t sed_crnn_ctx_bytes(const sed_dims* d);
int sed_crnn_forward(const sed_dims* d, const float* params, float* bn_running, int64_t* bn_tracked,
                     const float* x, int train, int update_bn, const uint64_t* seed_dev,
                     void* ctx, size_t ctx_bytes, float* strong, float* weak, void* stream);

/* The patch moments of conv block 0's train-mode BatchNorm (csrc/blk0.hip: the statistics of BatchNorm2d(Conv2d(1, C, 3)(x)),
 * baseline/models/CNN.py:46-55, follow from the 9 + 45 first / second moments of the 3x3 input patch) depend on the batch only.
 * sed_crnn_forward computes them at its head (train = 1 / 3); a caller that already holds the NEXT batch while a step runs -
 * one batch ahead like the reference's DataLoader workers (DataLoad.py:47-186) - calls this beside that step and then passes
 * train | 4 to the forward that consumes them (same ctx): the launch leaves the head of the critical chain.  Bit-identical. */
int sed_crnn_moments(const sed_dims* d, const float* x, void* ctx, size_t ctx_bytes, void* stream);

/* Backward of the above in train mode (autograd of main.py:153 loss.backward()).
 *   d_strong/d_weak  gradients w.r.t. the two outputs
 *   grads            flat, same layout as params; OVERWRITTEN with dLoss/dparams
 *   ws               scratch, sed_crnn_bwd_ws_bytes(d)
 *   parts            3 = whole backward (what a single-GPU caller uses).  A data-parallel caller splits it so that
 *                    the all-reduce of the GRU + heads gradient bucket overlaps the conv-block backward:
 *                      1  heads + BiGRU incl. their weight gradients (the rnn/dense tail of grads is complete)
 *                      5  heads + BiGRU data-gradient chain only; the tail's weight gradients are left to a
 *                         later parts = 8 call on the same ws (any stream ordered after this call)
 *                      8  the weight gradients deferred by 5 (head column sum + GRU dW/db GEMMs)
 *                      2  conv blocks (the cnn head of grads; needs 1 or 5 to have run on the same ws)
 * Concurrency: the library forks its weight-gradient kernels onto a helper stream it owns - one helper stream and one
 * fork/join event pair per (device, caller stream), created under a mutex by sed_stream_prepare(stream) or on first
 * use (event fork/join, capturable) - so calls on different caller streams, from different host threads or on
 * different devices never share state.  Call sed_stream_prepare for a stream BEFORE capturing it into a hipGraph. */
int sed_stream_prepare(void* stream);
/* Destroys what sed_stream_prepare (or first use) created for `stream` on the current device - two helper streams, three
 * events, a pending fork hook.  Call it when a stream the library has seen goes away (a training step object that owned its
 * capture / teacher / collective streams is deleted: train.MeanTeacherStep.close()); without it every stream ever passed in
 * keeps two live helper streams for the life of the process, and graph branches of later steps end up sharing hardware queues
 * with them (measured: the fifth step built in one process ran at 0.90 instead of 0.66 ms).  Precondition: no library work in
 * flight or under capture on `stream`.  hipGraphs captured earlier stay valid (a capture records nodes and edges, not the
 * helper streams).  Synchronises the helper streams - the only blocking call of this ABI.  Unknown stream: no-op, returns 0. */
int sed_stream_release(void* stream);
/* One-shot fork hook: the NEXT sed_crnn_forward enqueued on `stream` calls fn(user) - on the calling host thread, once,
 * then forgets it - after enqueueing its last conv-block kernel and before its first recurrence kernel.  The recurrent half
 * of CRNN.forward (models/CRNN.py:74-84: BiGRU, attention heads) occupies one workgroup per (clip, direction) - a fraction of
 * the chip - so a callback that forks a second stream off `stream` there (event record + wait, capturable) runs independent
 * work - the NEXT batch's feature extraction, the job of the reference's DataLoader workers (DataLoad.py:47-186) - on
 * otherwise idle CUs.  fn must not call back into sed_crnn_forward on the same stream.  fn == NULL clears the hook. */
int sed_crnn_fork_callback(void* stream, void (*fn)(void*), void* user);
size_t sed_crnn_bwd_ws_bytes(const sed_dims* d);
int sed_crnn_backward(const sed_dims* d, const float* params, const float* x, const uint64_t* seed_dev,
                      void* ctx, size_t ctx_bytes, const float* d_strong, const float* d_weak,
                      float* grads, void* ws, size_t ws_bytes, int parts, void* stream);
/* sed_crnn_backward with one more upstream gradient: d_att [B][T/8][nclass] fp32 = dLoss/d(sof), sof the attention as
 * sed_crnn_attention returns it (after the clamp).  The heads backward adds it to the gradient that reaches sof through the
 * pooling, in front of the clamp's pass mask: ds = (dnum * strong + dden + d_att) * pass; nothing else differs, every other
 * argument, `parts` value, sed_dims.dtype and both kernel sets as for sed_crnn_backward.  d_att == NULL enqueues exactly
 * what sed_crnn_backward enqueues (bit-identical gradients).  A loss on anything formed from the attention outside the
 * network - the recording-level tag of sed_stitch_weak - reaches the parameters through it. */
int sed_crnn_backward_att(const sed_dims* d, const float* params, const float* x, const uint64_t* seed_dev,
                          void* ctx, size_t ctx_bytes, const float* d_strong, const float* d_weak, const float* d_att,
                          float* grads, void* ws, size_t ws_bytes, int parts, void* stream);

/* One-time initialisation of a FRESH ctx and / or backward workspace (either pointer may be NULL): clears the few
 * regions the library reads before it writes them - the wide model's cluster recurrence keeps launch epochs and tagged
 * exchange granules in both buffers, and ctx holds the sticky "gru_err" counter that a timed-out cross-workgroup wait
 * increments (never cleared by a forward; read it through sed_crnn_ctx_view).  Buffers that are reused across calls
 * (train.MeanTeacherStep) need it once; the autograd path (crnn.py, a new ctx per CRNN.forward as in
 * models/CRNN.py:59-84 called from main.py:91) calls it per allocation.  hipMemsetAsync on `stream`: capturable. */
int sed_crnn_buffers_init(const sed_dims* d, void* ctx, size_t ctx_bytes, void* ws, size_t ws_bytes, void* stream);

/* Debug / test access to intermediates inside ctx: name in {"p0","y1","p1","y2","p2","gru0",
 * "gru1","wz0","mean0","scale1","shift1",...}. Returns 0 and fills offset/bytes, or <0. */
int sed_crnn_ctx_view(const sed_dims* d, const char* name, size_t* offset, size_t* bytes);

/* The attention of the forward that filled ctx: att [B][T/8][nclass] fp32 = sof = clamp(softmax(dense_softmax(x), dim = -1),
 * 1e-7, 1) (models/CRNN.py:79), the weights the heads pooled `weak` with.  Rebuilt from the attention logits that every
 * sed_crnn_forward keeps in ctx (any `train`, any sed_dims.dtype, both kernel sets) with the heads kernel's own arithmetic
 * and summation order; the forward's launches are unchanged.  One launch on `stream`, no allocation, hipGraph-capturable.
 * sed_dims outside the hot path, a null pointer or ctx_bytes < sed_crnn_ctx_bytes(d): SED_ERR_BAD_ARG before any launch.
 * Overlapping windows' weak tags cannot be combined without it: see sed_stitch_weak. */
int sed_crnn_attention(const sed_dims* d, const void* ctx, size_t ctx_bytes, float* att, void* stream);

/* ---- mean-teacher loss ---------------------------------------------------------------------
 * Replaces the loss block of main.train (main.py:93-145): target_weak = target.max(-2),
 * BCE(weak[wm]) + BCE(strong[sm]) + w*MSE(strong, strong_ema) + w*MSE(weak, weak_ema), with
 * w = state->cons_weight, and its gradient w.r.t. the student outputs.
 *   masks are the reference's Python slices (main.py:241,247) as [lo, hi) row ranges; lo==hi
 *   disables the term (weak_mask / strong_mask = None).
 *   BCE is nn.BCELoss with its two clamps: each logarithm at -100, the gradient (p - t) / max((1 - p) p, 1e-12); a posterior of
 *   exactly 0 or 1 gives finite terms and gradients.  The posteriors come from the heads' fast sigmoid (csrc/common.h
 *   sigmoidf_fast = v_rcp(1 + v_exp(-z)), flushing denormals): for a logit in -88 .. -104 torch keeps a denormal posterior and
 *   an unclamped logarithm where the kernels give exactly 0 and the -100 clamp - the one zone where the two differ by more
 *   than rounding (tests/test_gpu_heads_regimes.py pins both sides of it, not the zone).
 *   losses: float[SED_LOSS_FLOATS(B)], ZERO-INITIALISED by the caller once (not per call):
 *     [0,8) = {loss, weak_bce, strong_bce, cons_strong, cons_weak, weak_ema_bce, strong_ema_bce,
 *              cons_weight}  (the meters of main.py:106-149);
 *     the rest is scratch (per-clip partial sums + the ticket of the last-workgroup reduction). */
#define SED_LOSS_FLOATS(B) (8 + 8 * (B) + 8)
int sed_mt_loss(const sed_dims* d, const float* strong, const float* weak, const float* strong_ema,
                const float* weak_ema, const float* target, int weak_lo, int weak_hi, int strong_lo,
                int strong_hi, const sed_step_state* state_dev, float* losses, float* d_strong,
                float* d_weak, void* stream);

/* sed_mt_loss + sed_crnn_backward in one call (what MeanTeacherStep uses): the loss gradient w.r.t. the student's
 * posteriors needs no reduction over the batch, so the heads-backward kernel forms it per clip on the fly and the
 * separate loss kernel (12 us on the critical path between forward and backward) disappears.  The student's
 * posteriors are the ones sed_crnn_forward(train=1) left in ctx; `losses` as for sed_mt_loss (same meters; summed in
 * a different order, so equal to rounding); d_strong / d_weak: optional outputs (may be NULL); parts: 1 or 3. */
/* advance_state != 0: the kernel that finishes the loss also advances *state_dev to the next step - what
 * sed_step_state_advance would do after the update, minus the update's own derived fields (ema_alpha, adam_step_size,
 * adam_sqrt_bc2), which are (re)derived here for THIS step and are therefore valid for the sed_adam_ema call that
 * follows.  A caller that passes advance_state must not call sed_step_state_advance for this step as well. */
int sed_mt_loss_backward(const sed_dims* d, const float* params, const float* x, const uint64_t* seed_dev,
                         void* ctx, size_t ctx_bytes, const float* strong_ema, const float* weak_ema,
                         const float* target, int weak_lo, int weak_hi, int strong_lo, int strong_hi,
                         sed_step_state* state_dev, int advance_state, float* losses, float* d_strong, float* d_weak,
                         float* grads, void* ws, size_t ws_bytes, int parts, void* stream);

/* The student's half of one train step after its forward with deferred heads (sed_crnn_forward(..., strong = NULL,
 * weak = NULL)): output heads (models/CRNN.py:74-81) -> losses (main.py:93-145) -> backward (main.py:152-153).  Arguments as
 * sed_mt_loss_backward plus `strong` / `weak`, which RECEIVE the student's posteriors.  With n_RNN_cell = 64 and T / 8 <= 128
 * the three run as the prologue phase of the top BiGRU layer's backward-recurrence kernel (csrc/hfuse.h): the heads' forward
 * kernel, the cross-queue join in front of the loss and the heads' backward kernel - 40 us of every step on 24 of 256 CUs -
 * leave the critical chain; the meters' sums over the clips and the step-state advance are finished by a small kernel on the
 * library's weight-gradient stream (they are complete when the call's work is, like everything else).  Other geometries (and
 * d_strong / d_weak != NULL) take the separate kernels inside this call; results are bit-identical either way except for the
 * meters (summation order).  Supervised loop (main_simple_CRNN.py): strong_ema == strong and weak_ema == weak. */
int sed_mt_step_backward(const sed_dims* d, const float* params, const float* x, const uint64_t* seed_dev,
                         void* ctx, size_t ctx_bytes, float* strong, float* weak, const float* strong_ema,
                         const float* weak_ema, const float* target, int weak_lo, int weak_hi, int strong_lo, int strong_hi,
                         sed_step_state* state_dev, int advance_state, float* losses, float* d_strong, float* d_weak,
                         float* grads, void* ws, size_t ws_bytes, int parts, void* stream);

/* ---- data-parallel gradient all-reduce over peer-mapped memory (csrc/p2p.hip) --------------------------------------------
 * New capability (the reference is single-process); what it serves is the per-rank batch contract of main.py:238-247 /
 * DataLoad.py:562-571 and the mean gradient of main.py:152-154.  One launch = reduce-scatter + all-gather with direct loads /
 * stores between the W ranks of one node (xGMI is point-to-point: every peer is one hop), sums formed in rank order on every
 * rank (bit-identical replicas), capturable into the step's hipGraph, every cross-rank wait bounded (sticky error counter, NaN
 * poisoning).
 *   sed_p2p_buffer_bytes(n)  size of a rank's communication buffer for messages of up to n floats
 *   sed_p2p_alloc            allocates (fine-grained device memory; falls back to hipMalloc), zeroes and exports one (the
 *                            exception stated under Conventions at the top); handle = 64 bytes.  The wait budget of the kernel's
 *                            cross-rank waits is set here: SED_P2P_TIMEOUT_S seconds, default 600
 *   sed_p2p_configure        (blocking) timeout_s > 0: new wait budget; host_err: host address of a 4-byte word in pinned,
 *                            mapped host memory that every timed-out wait increments too (polled by the host per step
 *                            without synchronising); clear_host_err != 0 removes it
 *   sed_p2p_open / _close    map / unmap a peer's buffer from its handle (hipIpcOpenMemHandle); _free releases one's own
 *   sed_p2p_can_access(dev)  1 if the current device can map device dev's memory
 *   sed_p2p_allreduce        in-place sum of data[0, n) over the ranks; bufs[world] = every rank's buffer as mapped HERE
 *                            (bufs[rank] = own); same n_floats_max and workgroups (0 = one per 2 K floats of n_floats_max, 32 .. 128) on every rank; every rank enqueues the
 *                            same sequence of calls
 *                            A cross-rank wait that exhausts its budget raises the sticky counter AND fills this launch's
 *                            output (the local bucket, and the slice this rank broadcasts) with NaN: a timed-out all-reduce
 *                            never looks like a result
 *   sed_p2p_errors           the sticky count of timed-out waits (blocking 4-byte read) */
size_t sed_p2p_buffer_bytes(long long n_floats_max);
int sed_p2p_alloc(size_t bytes, int fine_grained, void** ptr_out, void* handle_out, int* fine_grained_out);
int sed_p2p_open(const void* handle, void** ptr_out);
int sed_p2p_close(void* peer_ptr);
int sed_p2p_free(void* own_ptr);
int sed_p2p_can_access(int peer_device);
int sed_p2p_errors(const void* own_ptr, unsigned int* out);
int sed_p2p_configure(void* own_ptr, double timeout_s, unsigned int* host_err, int clear_host_err);
int sed_p2p_allreduce(float* data, long long n, int rank, int world, void* const* bufs, long long n_floats_max,
                      int workgroups, void* stream);

/* ---- optimiser + EMA -----------------------------------------------------------------------
 * Replaces optimizer.step() of torch.optim.Adam(lr, betas) (main.py:154,289-290) fused with
 * update_ema_variables (main.py:45-49,156-157) over the flat buffers. grad_scale multiplies
 * the gradient first (1/world_size after a sum all-reduce; 1 otherwise).  ema_params may be NULL:
 * plain Adam, the optimizer.step() of the supervised loop (main_simple_CRNN.py:75). */
int sed_adam_ema(int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                 float* ema_params, const sed_step_state* state_dev, float grad_scale, void* stream);

/* Plain EMA for the drop-in update_ema_variables(model, ema_model, alpha, global_step) call. */
int sed_ema_update(int64_t n, const float* params, float* ema_params, float alpha, void* stream);

/* Initialise / advance the device step state (one tiny kernel; graph-capturable).
 * init: global_step = 0, opt_step = 1 and the derived fields of the first step.
 * advance: called once at the END of each train step; moves to the next step's values. */
int sed_step_state_init(sed_step_state* state_dev, uint64_t base_seed, int64_t rampup_length,
                        double lr, double beta1, double beta2, double eps, double ema_decay,
                        double max_cons_cost, void* stream);
int sed_step_state_advance(sed_step_state* state_dev, void* stream);
/* Change the user-settable fields of a live state and re-derive the fields of the CURRENT step: flags bit 0 = base_seed
 * (a data-parallel rank folds its rank into the seed so that replicas draw different dropout masks, also after a
 * checkpoint written by rank 0 was loaded), bit 1 = lr (baseline/main.py:289 sets it once; adjust_learning_rate,
 * utils/utils.py:227-241, is dead code in main.py:81 but an optimizer whose lr changed between epochs is honoured). */
int sed_step_state_update(sed_step_state* state_dev, uint64_t base_seed, double lr, int flags, void* stream);
/* main.train recomputes global_step = epoch * len(train_loader) + i from its epoch argument at every call (baseline/main.py:74):
 * sets the counter the ramp-up (main.py:74-78), the EMA alpha (main.py:155-157) and the dropout keys are derived from, and
 * re-derives them; the optimiser's own step counter (Adam bias correction) is untouched. */
int sed_step_state_set_global_step(sed_step_state* state_dev, int64_t global_step, void* stream);

/* ---- feature front-end ---------------------------------------------------------------------
 * sed_mel_spec replaces DatasetDcase2019Task4.calculate_mel_spec (DatasetDcase2019Task4.py:
 * 197-231) with save_log_feature=False: symmetric Hamming-n_fft STFT (center, reflect pad),
 * magnitude, mel_basis @ |S|, transposed -> mel [n_clips][frames][n_mels] fp32 (linear).
 *   wave       [n_clips][n_samples] fp32
 *   window     [n_fft] fp32 (np.hamming(n_fft))
 *   mel_basis  [n_mels][n_fft/2+1] fp32 (librosa.filters.mel(..., htk=False, norm=None))
 *   n_fft must be 2048; frames = 1 + n_samples / hop.                                         */
size_t sed_mel_spec_ws_bytes(int n_clips, int n_samples, int hop, int n_fft, int n_mels);
int sed_mel_spec(const float* wave, int n_clips, int n_samples, int hop, int n_fft,
                 const float* window, const float* mel_basis, int n_mels, float* mel,
                 void* ws, size_t ws_bytes, void* stream);
/* The two halves of sed_mel_spec for callers that extract features batch after batch (the reference builds np.hamming and
 * librosa.filters.mel once per process too, DatasetDcase2019Task4.py:211-228):
 *   sed_mel_tables  fills ws with everything that depends on (window, mel_basis) only: the W_2048 table, the float64
 *                   window (window == NULL: np.hamming(n_fft) generated in float64), the support of every mel band and the
 *                   band-compressed filterbank;
 *   sed_mel_frames  the STFT + mel projection proper, reading a ws prepared by sed_mel_tables with the SAME mel_basis.
 *                   One persistent launch of at most max_workgroups workgroups (<= 0: one per CU); each occupies one CU
 *                   completely, so a caller that runs it beside other work (features of batch k + 1 during train step k)
 *                   decides how much of the chip the front-end may take.  Results do not depend on max_workgroups.
 *                   fft_dtype selects the butterfly arithmetic, explicitly (never chosen silently, like sed_dims.dtype):
 *                     SED_FFT_F64  float64, what librosa computes in (soundfile hands it float64 audio): the parity mode
 *                     SED_FFT_F32  float32 butterflies, twiddles / window generated in float64 and rounded once.  A stated
 *                                  reduced-precision mode for the bf16 train step of BASELINE.json configs[2]; measured
 *                                  error bounds (dB on the features, posteriors at B = 64) in tests/test_gpu_features.py. */
#define SED_FFT_F64 0
#define SED_FFT_F32 1
int sed_mel_tables(int n_fft, const float* window, const float* mel_basis, int n_mels, void* ws, size_t ws_bytes,
                   void* stream);
int sed_mel_frames(const float* wave, int n_clips, int n_samples, int hop, int n_fft, const float* mel_basis,
                   int n_mels, float* mel, const void* ws, size_t ws_bytes, int fft_dtype, int max_workgroups,
                   void* stream);

/* sed_logmel_transform replaces the per-sample transform chain of get_transforms
 * (utils/utils.py:397-412): [AugmentGaussianNoise] -> ApplyLog (librosa.amplitude_to_db, amin
 * 1e-5, top_db 80 per clip) -> PadOrTrunc(max_frames) -> ToTensor -> Normalize(scaler)
 * (DataLoad.py:262-287,189-207,210-259,290-321,324-350; Scaler.normalize Scaler.py:99-105).
 *   mel     [n_clips][frames][n_mels] linear mel
 *   mean/std  [n_mels] float64 (Scaler.mean_/std_ are float64) or NULL (no Normalize)
 *   out_clean [n_clips][max_frames][n_mels]; out_noisy same or NULL (no augmentation)
 *   seed_dev  Philox key for the teacher noise |N(0, 0.25)| (DataLoad.py:285)
 *   ws        scratch, sed_logmel_transform_ws_bytes(n_clips): per-clip partial maxima (the per-clip top_db clamp is
 *             a two-pass reduction spread over the whole chip)                                  */
size_t sed_logmel_transform_ws_bytes(int n_clips);
/* Advances a device-resident 64-bit noise key by one draw (key += 0x9E3779B97F4A7C15), in stream order: the state of
 * AugmentGaussianNoise's generator (DataLoad.py:189-207 draws from numpy's global RNG once per sample) for callers that
 * run the transform chain on a stream of their own, ahead of the train step. */
int sed_seed_advance(uint64_t* key_dev, void* stream);
/*   math_dtype  SED_FFT_F64: the reference's arithmetic (numpy float64 for log10, the noise and the normalisation);
 *               SED_FFT_F32: the front-end's stated fp32 mode - fp32 log10 / Box-Muller / normalisation (bounds asserted in
 *               tests/test_gpu_features.py next to the fp32 STFT's)                                                          */
int sed_logmel_transform(const float* mel, int n_clips, int frames, int n_mels, int max_frames,
                         const double* mean, const double* std, const uint64_t* seed_dev,
                         float* out_clean, float* out_noisy, void* ws, size_t ws_bytes, int math_dtype, void* stream);
/* sed_gather_logmel_transform: the same transform chain on B clips GATHERED from a device-resident pool of linear mel
 * (features stored once in HBM, every batch of an epoch addressed through a device index list).
 *   pool        every clip's linear mel, fp32, concatenated along frames; clip i = frames [clip_offset[i],
 *               clip_offset[i] + clip_frames[i]) x n_mels, of any length (the top_db clamp covers the whole clip, then
 *               pad / truncate to max_frames as above)
 *   idx [B]     device int32 pool clips of this batch (repeats allowed); NOT range-checked by the kernel - the caller
 *               validates every entry against [0, n_pool) when it builds its index tables
 *   max_clip_frames  L_max, the longest clip of the pool: noise counters of batch position b, element e are b * S + e with
 *               S = L_max * n_mels (Philox pair (b S + e) >> 1) - with equal-length clips this is sed_logmel_transform's
 *               layout, bit for bit
 *   tgt_pool [n_pool][tgt_elems], out_target [B][tgt_elems]: the clips' encoded targets, copied by the same launch
 *               (both NULL: no targets)
 *   mean/std, seed_dev, out_clean, out_noisy (NULL: validation form), ws = sed_logmel_transform_ws_bytes(B), math_dtype:
 *               as sed_logmel_transform                                                                                  */
int sed_gather_logmel_transform(const float* pool, const int64_t* clip_offset, const int32_t* clip_frames, int n_pool,
                                int max_clip_frames, const int32_t* idx, int B, int n_mels, int max_frames,
                                const double* mean, const double* std, const uint64_t* seed_dev, float* out_clean,
                                float* out_noisy, const float* tgt_pool, int tgt_elems, float* out_target, void* ws,
                                size_t ws_bytes, int math_dtype, void* stream);
/* sed_gather_window_logmel_transform: the same transform chain on B WINDOWS that start inside pool items (training on
 * recordings longer than one clip: crops of `max_frames` feature frames, their labels sliced from the item's timeline).
 *   pool, clip_offset, clip_frames, n_pool   as above: item i = frames [clip_offset[i], clip_offset[i] + clip_frames[i])
 *   win [B][2]  device int32 {item, start3}.  Window b is item i = win[b][0], feature frames [s, s + n) with
 *               s = win[b][1] * pool_ratio and n = min(max_frames, clip_frames[i] - s).  Everything
 *               sed_gather_logmel_transform does to a clip is done to these n frames: the top_db clamp is taken over the
 *               window's own real frames (no frame outside it changes a byte), padding is 0 dB after the log, then the
 *               normalisation - bit for bit what the same frames give as a pool clip of their own
 *   max_win_frames  noise counters of batch position b, element e are b * S + e with S = max_win_frames * n_mels; the
 *               caller gives max_win_frames >= min(max_frames, longest item) (with every window full: sed_logmel_transform's
 *               layout)
 *   label_pool  every item's label timeline [label_rows[i]][nclass] fp32 at label-frame rate, concatenated along rows from
 *               row label_offset[i] (int64);
 *               out_target[b][u][c] = label_pool[(label_offset[i] + start3 + u) * nclass + c]  for start3 + u < label_rows[i],
 *                                   = 0.0f beyond.  Values are copied exactly (soft labels, the unlabelled stream's -1).
 *               label_pool, label_offset, label_rows, out_target: all NULL (no targets) or all non-NULL
 *   safety      inside the kernel item is clamped to [0, n_pool) and start3 so that s is in [0, clip_frames[i] - 1]: no
 *               table content can address outside the pool or the label pool (the caller still validates its tables - a
 *               clamped row is a wrong batch, not a fault)
 *   mean/std, seed_dev, out_clean, out_noisy (NULL: no noise), ws = sed_logmel_transform_ws_bytes(B), math_dtype: as
 *               sed_logmel_transform.  Limits: pool_ratio >= 1, max_frames * n_mels < 2^31, T3 * nclass < 2^31,
 *               B * max_win_frames * n_mels < 2^32.  Two launches on `stream`, no allocation, no atomics, no host
 *               synchronisation, hipGraph-capturable.
 * Not provided: crop starts finer than one label frame.                                                                   */
int sed_gather_window_logmel_transform(const float* pool, const int64_t* clip_offset, const int32_t* clip_frames, int n_pool,
                                       int max_win_frames, const int32_t* win, int B, int n_mels, int max_frames,
                                       int pool_ratio, const double* mean, const double* std, const uint64_t* seed_dev,
                                       float* out_clean, float* out_noisy, const float* label_pool,
                                       const int64_t* label_offset, const int32_t* label_rows, int T3, int nclass,
                                       float* out_target, void* ws, size_t ws_bytes, int math_dtype, void* stream);

/* ---- train-time batch augmentation -------------------------------------------------------------
 * Mixup of features and targets, a circular time shift of features and strong targets, and SpecAugment-style time /
 * frequency masks, applied to one gathered batch.  The reference has no such code: the definitions below are the
 * project's own, and no external package's parity is claimed; pinned is exact (bitwise) agreement with an independent
 * numpy float32 statement of them (tests/augment_np.py).
 *   x [B][T][M]        fp32 features (gathered, log-scaled, padded, normalised; [B][1][T][M] is the same memory)
 *   x_ema [B][T][M]    the teacher's noisy copy, or NULL (then out_x_ema is NULL too)
 *   target [B][T3][NC] the encoded targets, or NULL (then out_target is NULL too and T3 / NC are ignored)
 *   table [B][8]       device int32; the row of clip b is {partner, lambda_bits, shift_x, shift_y, f0, fw, t0, tw},
 *                      lambda_bits the bit pattern of an fp32 lambda
 * With r(s, n) = ((s mod n) + n) mod n, p_b = partner of b, s = the named shift column:
 *   mix(A, b, t, ., s) = lambda_b (x) A[b, r(t - s_b, n), .]  (+)  (1 - lambda_b) (x) A[p_b, r(t - s_{p_b}, n), .]
 *   out_x[b,t,m]      = 0                          if f0_b <= m < f0_b + fw_b  or  t0_b <= t < t0_b + tw_b
 *                     = mix(x, b, t, m, shift_x)   otherwise                                    (n = T)
 *   out_x_ema[b,t,m]  = the same with x_ema (same partner, lambda, shift and masks: only the noise differs)
 *   out_target[b,u,c] = mix(target, b, u, c, shift_y)                     (n = T3; masks never touch targets)
 * Rules:
 *   - each clip is rolled by ITS OWN shift before mixing: the partner contributes its own shifted clip; the partner's
 *     lambda and masks play no part;
 *   - masks are applied last, in output coordinates; the fill value is 0.0f (the band mean after normalisation);
 *   - (x), (+) and 1 - lambda are individually rounded fp32 operations, never contracted into an FMA;
 *   - when p_b == b or lambda_b == 1.0f the partner is NOT READ and the value is the rolled clip's own, copied exactly;
 *   - any int32 shift is legal and is reduced as above;
 *   - mask intervals are clipped to the tensor; fw <= 0 / tw <= 0: no mask;
 *   - partner is clamped to [0, B) inside the kernel, so no table content can address outside the batch;
 *   - labels are mixed softly only (no clamp(a + b) mode).
 * Output buffers must not overlap input buffers (the table included) or each other: the address ranges are checked
 * and SED_ERR_BAD_ARG is returned before anything is launched.  16-byte loads / stores when M % 4 == 0 (NC % 4 == 0
 * for the targets) and the bases are 16-byte aligned, a scalar path otherwise.  Limits: B <= 65535, T * M < 2^31,
 * T3 * NC < 2^31.  One launch on `stream`, no allocation, no atomics, hipGraph-capturable. */
int sed_batch_augment(const float* x, const float* x_ema, const float* target, const int32_t* table, int B, int T,
                      int M, int T3, int NC, float* out_x, float* out_x_ema, float* out_target, void* stream);

/* Resampling step of read_audio (utils/utils.py:175-193: librosa.resample(audio, orig_sr, target_sr),
 * res_type "kaiser_best" = resampy's windowed-sinc interpolation, then fix_length).
 *   x [n_clips][n_in] fp64 (soundfile.read returns float64; channels already averaged)
 *   ratio = target_sr / orig_sr;  interp_win [nwin] fp64 = right half of the Kaiser-windowed sinc with
 *   num_table samples per zero crossing, already multiplied by ratio when ratio < 1 (as resampy does)
 *   time_reg [int(n_in * ratio)] fp64 = resampy's running sum 0, 1/ratio, 1/ratio + 1/ratio, ... (exactly as a
 *   sequential loop rounds it: numpy.cumsum), or NULL for t * (1/ratio)
 *   y [n_clips][n_out] fp64, n_out = ceil(n_in * ratio); samples past int(n_in * ratio) are 0.       */
int sed_resample(const double* x, int n_clips, int n_in, double ratio, const double* interp_win, int nwin,
                 int num_table, const double* time_reg, double* y, int n_out, void* stream);

/* Scaler statistics (baseline/utils/Scaler.py:34-87 `means`): ADDS sum(x) and sum(x^2) per column of
 * x [n_rows][n_cols] (fp32, e.g. log-mel frames x mel bands) to sums[0..n_cols) / sums[n_cols..2n_cols)
 * (fp64, zero them before the first batch); n_cols must divide 256.  mean_ = sums[0] / rows,
 * mean_of_square_ = sums[1] / rows over the whole set (equal clip shapes, as the reference requires). */
int sed_scaler_stats(const float* x, long long n_rows, int n_cols, double* sums, void* stream);

/* ---- inference post-processing ---------------------------------------------------------------
 * Replaces the per-clip host loop of get_predictions (evaluation_measures.py:203-231) after the
 * forward: ProbabilityEncoder().binarization(global_threshold) -> scipy.ndimage median_filter
 * (median_window, 1) (mode "reflect") -> ManyHotEncoder.decode_strong / DecisionEncoder
 * .find_contiguous_regions (utils/utils.py:146-162), for a whole batch of strong posteriors.
 *   strong     [n_clips][T][nclass] fp32 (output of sed_crnn_forward), T <= 2048
 *   binary     [n_clips][T][nclass] uint8 filtered decisions, or NULL
 *   ev_count   [n_clips][nclass] int32: events per (clip, class)
 *   ev_pairs   [n_clips][nclass][max_events][2] int32: (onset, offset) in output frames, offset
 *              exclusive, in time order; max_events >= ceil(T / 2)                               */
int sed_postprocess(const float* strong, int n_clips, int T, int nclass, float threshold,
                    int median_window, uint8_t* binary, int32_t* ev_count, int32_t* ev_pairs,
                    int max_events, void* stream);

/* ---- long-recording inference: blend of overlapping windows + decode of the whole timeline --------
 * A recording longer than one clip is cut into overlapping windows of T3 label frames, hop3 label frames apart; every
 * window goes through the forward on its own.  sed_stitch_decode blends the windows' strong posteriors into one
 * timeline per recording and runs ONE threshold, median filter and run-length decode over it.  The reference scores
 * 10-s clips only: the definitions below are the project's own; pinned is exact (bitwise for the blend) agreement with
 * an independent numpy float32 statement of them (tests/stitch_np.py) and with scipy / the restated dcase_util decode.
 *   win_strong [n_win][T3][NC]  fp32 window posteriors
 *   rec_win0   [n_rec + 1]      device int32: recording r owns windows rec_win0[r] .. rec_win0[r + 1] - 1, in time order;
 *                               n_win = rec_win0[n_rec]
 *   rec_frame0 [n_rec + 1]      device int64: recording r owns timeline frames rec_frame0[r] .. rec_frame0[r + 1] - 1
 *                               (L3_r of them); window j of a recording starts at its frame j * hop3
 *   thr [NC], win [NC]          device: per-class threshold (fp32) and median window (int32, 1 .. 63)
 * Blend.  Frame u of a recording is covered by its windows j with 0 <= v = u - j * hop3 < T3, taken in increasing j;
 *   weighting 0 (uniform): w = 1;  weighting 1 (taper): w = min(v + 1, T3 - v) (an integer held as fp32);
 *   P[u, c] = (sum_j w_j (x) p_j[v_j, c]) (/) (sum_j w_j): the numerator a sequential fp32 sum from 0.0f in increasing j,
 *   every product, sum and the division an individually rounded fp32 operation (nothing contracted into an FMA, the
 *   division correctly rounded); the weight sum is an exact integer.
 *   A frame covered by exactly ONE window takes that window's value copied exactly (no multiply, no divide): a
 *   single-window recording's timeline is its window's posteriors bit for bit.
 *   A recording whose windows do not cover all of its frames (inconsistent tables) raises err bit 32 and is not decoded.
 * Decode, per column (recording, class c): P > thr[c] -> scipy's median filter of win[c] frames, origin 0 ->
 *   find_contiguous_regions: the rules of sed_postprocess (one code, csrc/post.h).  The filter reflects at the
 *   recording's two ends only (repeatedly when the window is longer than the column).
 * Outputs.
 *   timeline [sum L3][NC]  fp32 blended posteriors, or NULL
 *   binary   [sum L3][NC]  uint8 filtered decisions, or NULL
 *   ev_ptr   [n_rec * NC + 1] int64 CSR offsets, column = rec * NC + c, columns in index order: ALWAYS the true counts
 *   ev_pairs [capacity][2] int32 (onset, exclusive offset) in timeline frames of the recording, in time order
 *   err      one int32, OR-ed (zero it first), bits as in sed_event_counts where they exist there:
 *              2 = more than `capacity` events in all: nothing is written at or beyond capacity and ev_pairs must be
 *                  treated as invalid (never a silently truncated table); capacity = sum_r NC * ceil(L3_r / 2) cannot overflow
 *              8 = a window outside 1 .. 63: that class is not decoded
 *             16 = malformed rec_win0 / rec_frame0 (not increasing, outside their own totals, or more tiles than the
 *                  workspace was sized for): the recording is not decoded
 *             32 = a recording with too few windows to cover it: not decoded
 *            No table content can make a kernel address outside win_strong [0, rec_win0[n_rec]) or the outputs
 *            [0, rec_frame0[n_rec]).  A caller must treat every output as invalid when err != 0.
 *   ws       sed_stitch_decode_ws_bytes(sum L3, n_rec, NC) bytes, 8-byte aligned: the per-tile onset counts
 * The work is split along time: a workgroup owns sed_stitch_tile_frames() frames of one recording plus a halo of at
 * most 63 / 2 + 1 frames per side; a count pass, two scans and a write pass (four launches on `stream`).  No host
 * synchronisation, no allocation, no float atomics, integer results bit-reproducible, hipGraph-capturable.  16-byte
 * accesses when NC % 4 == 0 and win_strong / timeline are 16-byte aligned, a scalar path otherwise.
 * Limits: sum L3 * NC < 2^31, NC <= 16, 1 <= hop3 <= T3 <= 4096 (the taper's weight sum stays exact). */
size_t sed_stitch_decode_ws_bytes(long long total_frames, int n_rec, int nclass);
int sed_stitch_tile_frames(void);
int sed_stitch_decode(const float* win_strong, const int32_t* rec_win0, const int64_t* rec_frame0, int n_rec, int T3,
                      int NC, int hop3, int weighting, const float* thr, const int32_t* win, float* timeline,
                      uint8_t* binary, int64_t* ev_ptr, int32_t* ev_pairs, long long capacity, void* ws,
                      size_t ws_bytes, int32_t* err, void* stream);

/* ---- K operating points from one blend ----------------------------------------------------------
 * sed_stitch_sweep decodes n_points = K operating points of the same window posteriors in one call: for every point k the
 * result is what sed_stitch_decode defines for thr[k], win[k] - the same blend with the same rounding, the same decision,
 * median filter (reflection only at a recording's two ends) and run-length decode (one code: csrc/post.h and the
 * blend of csrc/stitch.hip).  Nothing new is defined; pinned is byte-for-byte agreement with K calls of sed_stitch_decode.
 *   thr [K][NC] fp32, win [K][NC] int32  device: per (point, class) threshold and median window
 *   timeline [sum L3][NC]  fp32 blended posteriors or NULL: written once, it does not depend on k
 *   ev_ptr   [K * n_rec * NC + 1] int64: ONE CSR over all columns, column (k, rec, c) = (k * n_rec + rec) * NC + c, in index
 *            order, ALWAYS the true counts; point k is the columns k * n_rec * NC .. (k + 1) * n_rec * NC
 *   ev_pairs [capacity][2] int32 (onset, exclusive offset) in timeline frames of the recording, in time order
 *   There is no `binary` output: it would be K timelines.  Use sed_stitch_decode for the filtered decisions of one point.
 *   err      one int32, OR-ed, the bits of sed_stitch_decode: 2 = more events over ALL points than `capacity` (nothing is
 *            written at or beyond it, never a truncated table), 8 = a window outside 1 .. 63 at some (point, class): that
 *            column is not decoded, every other one is; 16 / 32 = malformed tables / an uncovered recording, as above.
 *            The address guarantee of sed_stitch_decode holds (one validation of the tables gates every access).
 *   ws       sed_stitch_sweep_ws_bytes(sum L3, n_rec, NC, K) bytes, 8-byte aligned; ws_bytes must be that value (the tile
 *            slots are derived from it: a size that is not a whole number of slots is refused)
 * Four launches whatever K is: count pass, column scan, pointer scan, write pass.  A workgroup blends the frames of its
 * tile ONCE per pass into LDS and takes the decisions, filters and counts of sed_stitch_sweep_point_group() points from
 * it; the grid's second dimension is the point group, each group blends again.  No host synchronisation, no allocation,
 * no float atomics (the only atomic is the OR into err), integer results bit-reproducible, hipGraph-capturable.
 * Limits, checked before any launch (SED_ERR_BAD_ARG): 1 <= K <= 4096, K * n_rec * NC < 2^26, sum L3 * NC < 2^31,
 * K * tile slots < 2^31, and NC, T3, hop3 as for sed_stitch_decode. */
size_t sed_stitch_sweep_ws_bytes(long long total_frames, int n_rec, int nclass, int n_points);
int sed_stitch_sweep_point_group(void);
int sed_stitch_sweep(const float* win_strong, const int32_t* rec_win0, const int64_t* rec_frame0, int n_rec, int T3,
                     int NC, int hop3, int weighting, int n_points, const float* thr, const int32_t* win,
                     float* timeline, int64_t* ev_ptr, int32_t* ev_pairs, long long capacity, void* ws, size_t ws_bytes,
                     int32_t* err, void* stream);

/* ---- two-threshold (hysteresis) decode, in the event domain -------------------------------------
 * A low threshold draws the event boundaries, a high threshold decides whether the event exists.  The definition is the
 * project's own; pinned is exact agreement with a plain-loop numpy statement (tests/hysteresis_np.py).  Per column (point
 * pair k, recording, class c), with thr_lo[k, c] <= thr_hi[k, c] and ONE median window win[k, c]:
 *   E_lo = the event list sed_stitch_decode defines for (thr_lo, win)
 *   E_hi = the event list sed_stitch_decode defines for (thr_hi, win)
 *   the result is the events [on, off) of E_lo, in order, for which some event of E_hi has on <= on_hi < off.
 * Why this is hysteresis: P > thr is monotone in thr and a binary median filter is monotone in its input, so for the same
 * window the filtered high decisions are a subset of the filtered low ones and every event of E_hi lies inside exactly one
 * event of E_lo.  Consequences:
 *   thr_hi == thr_lo reproduces sed_stitch_decode's table byte for byte (ev_ptr and the ev_pairs in front of ev_ptr's end).
 *   win == 1: frame-domain hysteresis with strict > on both thresholds - the connected runs of P > thr_lo that hold a frame
 *     with P > thr_hi (the semantics of skimage.filters.apply_hysteresis_threshold; no parity with that package is claimed,
 *     pinned is agreement with scipy.ndimage.label on the low decisions).
 *   win > 1: the rule is "filter both decisions, then select".  It is NOT "hysteresis, then filter": the two differ where
 *     the filter removes or merges what the frame-domain rule would have kept apart.
 *   NaN posteriors decide 0 at both thresholds (sed_stitch_decode's decision).
 * sed_events_hysteresis is the select alone, on two event tables that share one pairs array:
 *   lo_ptr, hi_ptr [n_cols + 1] int64  CSR offsets into pairs; for a sed_stitch_sweep of 2K points ordered [lo_0 .. lo_{K-1},
 *                                      hi_0 .. hi_{K-1}] they are ev_ptr and ev_ptr + K * n_rec * NC, n_cols = K * n_rec * NC
 *   pairs   [pairs_capacity][2] int32  (onset, exclusive offset), onsets strictly increasing inside a column
 *   out_ptr [n_cols + 1] int64         CSR offsets of the kept events, column for column: ALWAYS the true counts
 *   out_pairs [out_capacity][2] int32  the kept events; must not be `pairs`
 *   err     one int32, OR-ed (the bit meanings follow the stitch entries; zero it first or hand over the sweep's word):
 *              2 = more kept events than out_capacity: nothing is written at or beyond it, never a truncated table
 *             16 = a column whose bounds in lo_ptr or hi_ptr are not 0 <= ptr[c] <= ptr[c + 1] <= pairs_capacity: the column is
 *                  skipped (none of its events is kept).  A lo_ptr that is not non-decreasing can moreover leave events that
 *                  the bisection assigns to no column: they are dropped.  (A sweep that overflowed its own capacity raises
 *                  this bit here too: its ev_ptr runs past pairs_capacity.)
 *             64 = onsets that do not strictly increase inside a lo or a hi column: what that column keeps is undefined
 *            No table content can make a kernel address outside lo_ptr / hi_ptr [0, n_cols], pairs [0, pairs_capacity) or
 *            the outputs: every offset is validated before it is used as an index.  A caller must treat every output as
 *            invalid when err != 0.
 *   ws      sed_events_hysteresis_ws_bytes(pairs_capacity, n_cols) bytes, 8-byte aligned; ws_bytes must be that value
 * The work is flat over the indices of pairs, not over columns (a column has no length limit): a flag pass (a thread finds
 * the low column of its index by bisection over lo_ptr, bisects that column of the high table for the first onset >= its
 * own; wave ballots, one count per workgroup), a one-workgroup scan of the counts, a write pass.  Three launches on `stream`
 * whatever n_cols is (two when pairs_capacity is 0), grids sized from pairs_capacity.  No host synchronisation, no
 * allocation, no atomics but the OR into err, integer results bit-reproducible, hipGraph-capturable.
 * Limits, checked before any launch (SED_ERR_BAD_ARG; a wrong ws_bytes: SED_ERR_WORKSPACE): 1 <= n_cols < 2^26,
 * 0 <= pairs_capacity < 2^31, pairs / out_pairs / ws 8-byte aligned, no null pointer.
 * Not provided: "hysteresis, then filter", different windows for the two thresholds, a binary timeline. */
size_t sed_events_hysteresis_ws_bytes(long long pairs_capacity, long long n_cols);
int sed_events_hysteresis(const int64_t* lo_ptr, const int64_t* hi_ptr, const int32_t* pairs, long long pairs_capacity,
                          long long n_cols, int64_t* out_ptr, int32_t* out_pairs, long long out_capacity, void* ws,
                          size_t ws_bytes, int32_t* err, void* stream);

/* ---- minimum event length and gap merging, in the event domain --------------------------------------
 * The post-processing step applied to a decoded event table: drop events shorter than a minimum length, fuse events that a
 * short gap separates.  The definition is the project's own; pinned is exact agreement with a plain-loop numpy statement
 * (tests/event_process_np.py), which in turn agrees with a frame-domain (raster) statement on tables whose gaps are at
 * least 1 frame - every decode's.  Per column the events e_0 .. e_{n-1} are sorted and disjoint, on_i < off_i <= on_{i+1};
 * each column has two int32 parameters in label frames, min_len (m) and max_gap (g):
 *   DROP(m)   keeps the events with off - on >= m; m <= 0 keeps everything.
 *   MERGE(g)  joins two consecutive events of the list it receives when on_next - off_prev <= g; a maximal chain becomes
 *             one event [on_first, off_last).  g < 0 merges nothing, g = 0 fuses only abutting events.
 *   order 0   DROP then MERGE (the order of dcase_util's process_events(minimum_event_length, minimum_event_gap); no
 *             parity with that package is claimed).  The predecessor of a kept event is the previous KEPT event of its
 *             column: two events fuse across any number of dropped ones when their gap is at most g.
 *   order 1   MERGE then DROP: a binary closing followed by an opening.
 * The two orders differ: with m = 3, g = 2 the list [0,1) [2,3) [4,5) becomes empty under order 0 and [0,5) under order 1.
 * Both are idempotent.  With m <= 0 and g < 0 the output is the input byte for byte (ev_ptr, and the ev_pairs in front of its
 * end).  All differences are formed in 64 bits.  The median filter does not replace this step: its window couples the two
 * lengths, is symmetric and ends at 63.
 *   ev_ptr  [n_cols + 1] int64         CSR offsets into pairs; n_cols = K * n_rec * NC in the sweep's column order
 *                                      (k * n_rec + rec) * NC + c (K = 1: the table of sed_stitch_decode)
 *   pairs   [pairs_capacity][2] int32  (onset, exclusive offset)
 *   min_len, max_gap [K][NC] int32     device arrays; column col uses entry (col / (n_rec * NC)) * NC + col % NC
 *   order   0 or 1
 *   out_ptr [n_cols + 1] int64         CSR offsets of the result, column for column: ALWAYS the true counts
 *   out_pairs [out_capacity][2] int32  the result; must not be `pairs`.  It never holds more events than the input.
 *   err     one int32, OR-ed (the bits follow sed_events_hysteresis; zero it first or hand over the decode's own word):
 *              2 = more result events than out_capacity: nothing is written at or beyond it
 *             16 = a column whose bounds are not 0 <= ev_ptr[c] <= ev_ptr[c + 1] <= pairs_capacity: the column is skipped
 *                  (none of its events reaches the result).  An ev_ptr that is not non-decreasing can moreover leave
 *                  events that the bisection assigns to no column or to a neighbour: what the columns around the broken
 *                  entry hold is undefined.
 *             64 = a column that is not sorted and disjoint (some on >= off, or off > the next on): its result is undefined
 *            No table content can make a kernel address outside ev_ptr [0, n_cols], pairs [0, pairs_capacity), the
 *            parameter arrays or the outputs: every offset is validated before it is used as an index.  A caller must
 *            treat every output as invalid when err != 0.
 *   ws      sed_events_process_ws_bytes(pairs_capacity, n_cols) bytes, 8-byte aligned; ws_bytes must be that value
 * The work is flat over the indices of pairs (a column has no length limit), on two flags per index.  Order 0: A = kept,
 * B = head (a kept event without a kept predecessor in its column within g); a head's rank among the heads is its output
 * slot, it writes its onset there and its predecessor's offset into the slot before, and the thread of a column writes the
 * offset of the column's last kept event.  Order 1: A = head of a chain, B = a chain's last event whose merged event is at
 * least m long; it writes the pair (onset of the last A at or before it, its own offset) at its rank.  "The last A index in
 * front of p" is read from the ballot words of p's workgroup and a scanned per-workgroup maximum, so no thread's work grows
 * with a column, a chain or a run of dropped events.  Five launches on `stream` whatever K, n_cols and the column lengths
 * are (three when pairs_capacity is 0): flag A, scan (maximum), flag B, scan (sum; capacity check), write.  No host
 * synchronisation, no allocation, no atomics but the OR into err, integer results bit-reproducible, hipGraph-capturable.
 * Limits, checked before any launch (SED_ERR_BAD_ARG; a wrong ws_bytes: SED_ERR_WORKSPACE): 1 <= n_cols < 2^26,
 * n_cols a multiple of n_rec * NC, n_rec >= 1, NC >= 1, 0 <= pairs_capacity < 2^31, out_capacity >= 0, pairs / out_pairs /
 * ws 8-byte aligned, no null pointer.
 * Not provided: a binary timeline, different orders per class, minimum lengths in front of the median filter. */
size_t sed_events_process_ws_bytes(long long pairs_capacity, long long n_cols);
int sed_events_process(const int64_t* ev_ptr, const int32_t* pairs, long long pairs_capacity, long long n_cols,
                       int n_rec, int NC, const int32_t* min_len, const int32_t* max_gap, int order,
                       int64_t* out_ptr, int32_t* out_pairs, long long out_capacity,
                       void* ws, size_t ws_bytes, int32_t* err, void* stream);

/* ---- confidence scores of decoded events, and a select by score, in the event domain ------------------
 * Every decode leaves a CSR table of (onset, offset) pairs; sed_events_scores says how confident the posteriors were in each
 * event, sed_events_select keeps the events whose score exceeds a minimum.  The definitions are the project's own; pinned is
 * agreement with a plain-loop numpy statement (tests/event_scores_np.py): maxima bitwise, means within one fp32 step.
 *   timeline   [total_frames][NC] fp32   what a stitch entry writes, or any fp32 array of that shape.  A batch of n clips is
 *                                        n one-window recordings: `strong` reshaped, rec_frame0 = arange(n + 1) * T3
 *   rec_frame0 [n_rec + 1] int64         device: recording r owns the frames rec_frame0[r] .. rec_frame0[r + 1] - 1 (L3_r)
 *   ev_ptr [n_cols + 1] int64, ev_pairs [pairs_capacity][2] int32   a table in the sweep's column order, column (k, rec, c) =
 *                                        (k * n_rec + rec) * NC + c; n_cols = K * n_rec * NC (K = 1: sed_stitch_decode's)
 *   score_max, score_mean [pairs_capacity] fp32, indexed like ev_pairs; either may be NULL, not both.  Only the indices below
 *                                        ev_ptr[n_cols] that belong to a valid column are written.
 * Event i = [on, off) of column (k, rec, c), 0 <= on < off <= L3_rec, over P[u] = timeline[(rec_frame0[rec] + u) * NC + c],
 * on <= u < off:
 *   score_max[i]   the largest non-NaN P[u], NaN when every frame is NaN: a copy of an input value, no arithmetic.  (The sign
 *                  of a zero maximum is unspecified when the span holds both +0.0 and -0.0; a sigmoid gives no -0.0.)
 *   score_mean[i]  (float)(S / (double)(off - on)), S the fp64 sum of the P[u], each widened exactly.  A NaN frame makes the
 *                  mean NaN.  The order of the sum is a function of off - on alone - not of position, column or neighbours:
 *                  events of at most sed_events_scores_short_frames() frames are summed in increasing u; a longer one as 64
 *                  partial sums (partial l: the frames on + l, on + l + 64, ... in increasing order) combined by a fixed
 *                  butterfly.  So the mean is the same bits from call to call, under graph replay, and wherever the event lies.
 *   An event that sed_events_process fused across a gap is scored over its whole span, the gap's frames included.
 *   err    one int32, OR-ed, the family's bits:
 *            16 = a column whose bounds are not 0 <= ev_ptr[c] <= ev_ptr[c + 1] <= pairs_capacity, or a recording whose bounds
 *                 are not 0 <= rec_frame0[r] <= rec_frame0[r + 1] <= total_frames: nothing of it is read or written.
 *                 (As in sed_events_hysteresis, an ev_ptr that is not non-decreasing can moreover leave events that the
 *                 bisection assigns to no column: they are not scored.)
 *            64 = an event with on < 0, off > L3 or on >= off: its two scores are NaN and no frame of it is read
 *          No table content can make the kernel address outside timeline [0, total_frames * NC), ev_ptr [0, n_cols],
 *          ev_pairs or the outputs [0, pairs_capacity).
 * ONE launch on `stream` whatever K and the number of events are, flat over the indices of ev_pairs (grid sized from
 * pairs_capacity; none when it is 0).  No LDS tiles, no workspace, no host synchronisation, no allocation, no atomics but the
 * OR into err, hipGraph-capturable.
 * Limits, checked before any launch (SED_ERR_BAD_ARG): no null pointer except one of the two outputs, 1 <= NC <= 16,
 * n_rec >= 1, 1 <= n_cols < 2^26 a multiple of n_rec * NC, 0 <= pairs_capacity < 2^31, total_frames * NC < 2^31, ev_pairs
 * 8-byte aligned, no output overlapping an input or the other output.
 *
 * sed_events_select: an event of column (k, rec, c) is kept iff score[i] > min_score[k][c] - strict, like the decode's
 * P > thr; a NaN score is never kept.
 *   key        0: score_max decides, 1: score_mean.  The key's array must be given; the other one and its output go together
 *              or are both NULL.
 *   min_score  [K][NC] fp32, device
 *   out_ptr [n_cols + 1] int64   CSR offsets of the kept events, column for column: ALWAYS the true counts
 *   out_pairs [out_capacity][2], out_score_max / out_score_mean [out_capacity]   the kept events in order and their scores
 *              (copies); none of them may be its input
 *   err        2 = more kept events than out_capacity: nothing is written at or beyond it, never a truncated table
 *             16 = a column with broken bounds, as above: none of its events is kept
 *   ws         sed_events_select_ws_bytes(pairs_capacity, n_cols) bytes, 8-byte aligned; ws_bytes must be that value
 * Three launches (two when pairs_capacity is 0): a flag pass with wave ballots and one count per workgroup, a one-workgroup
 * scan, a write pass.  Limits and host checks as for sed_events_hysteresis, and n_rec, NC >= 1, n_cols a multiple of
 * n_rec * NC (SED_ERR_BAD_ARG; a wrong ws_bytes: SED_ERR_WORKSPACE).
 * Not provided: scoring without a written timeline, the position of the peak frame, scores weighted by the attention. */
int sed_events_scores_short_frames(void);
int sed_events_scores(const float* timeline, long long total_frames, const int64_t* rec_frame0, int n_rec, int NC,
                      const int64_t* ev_ptr, const int32_t* ev_pairs, long long pairs_capacity, long long n_cols,
                      float* score_max, float* score_mean, int32_t* err, void* stream);
size_t sed_events_select_ws_bytes(long long pairs_capacity, long long n_cols);
int sed_events_select(const int64_t* ev_ptr, const int32_t* ev_pairs, const float* score_max, const float* score_mean,
                      long long pairs_capacity, long long n_cols, int n_rec, int NC, int key, const float* min_score,
                      int64_t* out_ptr, int32_t* out_pairs, float* out_score_max, float* out_score_mean,
                      long long out_capacity, void* ws, size_t ws_bytes, int32_t* err, void* stream);

/* ---- recording-level weak tags of long recordings -------------------------------------------------
 * A window's `weak` is a ratio num / den of attention-pooled sums (models/CRNN.py:79-81); the ratios of overlapping
 * windows cannot be combined into the recording's ratio without the attention mass per frame.  sed_stitch_weak pools over
 * the whole blended timeline instead.  The definition is the project's own, like the blend; pinned is agreement with a
 * plain-loop statement that sums with math.fsum (tests/weak_np.py).  For recording r with L3_r timeline frames:
 *   P[u, c]  the blend of win_strong as sed_stitch_decode defines it (same rounding; a frame covered by one window is
 *            copied exactly)
 *   A[u, c]  the SAME blend applied to win_att [n_win][T3][NC]: the windows' attention sof (sed_crnn_attention)
 *   num[r, c] = sum_u (double)P[u, c] * (double)A[u, c]   (every product exact in fp64)
 *   den[r, c] = sum_u (double)A[u, c]                     both over u = 0 .. L3_r - 1, in fp64
 *   weak[r, c] = (float)(num / den)
 * Frames of the last window beyond L3_r never enter the sums.  No special case for den == 0 (0 / 0 gives NaN) or NaN
 * inputs (they propagate).  The order of the fp64 sums is fixed by the implementation and depends on (L3_r, NC) only -
 * not on scheduling, alignment or the other recordings; no float atomics: two calls give identical bytes.
 * Consequences: a single-window recording reproduces its window's clip-level weak up to the heads kernel's fp32
 * summation; with hop3 == T3 and L3 a multiple of T3, weak[r] is the den-weighted mean of the windows' tags.
 *   weak [n_rec][NC] fp32;  sums [n_rec][NC][2] fp64 (num, den) or NULL
 *   err  one int32, OR-ed (zero it first), the bits of sed_stitch_decode: 16 = malformed rec_win0 / rec_frame0 or more
 *        tiles than the workspace holds, 32 = a recording with too few windows to cover it.  The weak / sums rows of such
 *        a recording are written as NaN (never stale, never partial); the address guarantee of sed_stitch_decode holds for
 *        both window tensors.
 *   ws   sed_stitch_weak_ws_bytes(sum L3, n_rec, NC) bytes, 8-byte aligned: one (num, den) pair per (tile slot, class);
 *        ws_bytes must be that value (the tile slots are derived from it)
 * Two launches on `stream`: a tile pass (one workgroup per sed_stitch_tile_frames() frames of one recording blends both
 * tensors and reduces its fp64 products; no halo, no timeline is written) and a column pass.  16-byte accesses when
 * NC % 4 == 0 and both window tensors are 16-byte aligned, a scalar path otherwise (the same summation order).  No host
 * synchronisation, no allocation, hipGraph-capturable.
 * Limits, checked before any launch (SED_ERR_BAD_ARG): NC <= 16, 1 <= hop3 <= T3 <= 4096, sum L3 * NC < 2^31.
 * Tags per sub-span of a recording: sed_stitch_span_tags.  The backward through the pooled tag is sed_stitch_weak_backward. */
size_t sed_stitch_weak_ws_bytes(long long total_frames, int n_rec, int nclass);
int sed_stitch_weak(const float* win_strong, const float* win_att, const int32_t* rec_win0, const int64_t* rec_frame0,
                    int n_rec, int T3, int NC, int hop3, int weighting, float* weak, double* sums, void* ws,
                    size_t ws_bytes, int32_t* err, void* stream);

/* ---- backward through the pooled tag: training on recording-level tags ----------------------------
 * The transpose of sed_stitch_weak for a loss on weak[r, c]: the gradient w.r.t. both window tensors.  The inputs are the
 * forward's, plus
 *   sums   [n_rec][NC][2] fp64  the (num, den) pairs sed_stitch_weak returned for the same inputs
 *   g_weak [n_rec][NC]    fp32  dLoss/dweak
 * For recording r, class c, window j of that recording, local frame v, timeline frame u = j * hop3 + v < L3_r:
 *   P[u, c], A[u, c]  the blends of win_strong / win_att exactly as sed_stitch_decode defines them (one code)
 *   w = 1 (uniform) or min(v + 1, T3 - v) (taper);  W(u) = the integer sum of w over the windows covering u
 * and, every operation an individually rounded fp64 operation in this order (g = g_weak[r, c]),
 *   t  = num / den
 *   dP = ((double)g * (double)A[u, c]) / den
 *   dA = ((double)g * ((double)P[u, c] - t)) / den
 *   d_win_strong[j, v, c] = (float)((dP * (double)w) / (double)W)
 *   d_win_att[j, v, c]    = (float)((dA * (double)w) / (double)W)
 * (a frame covered by one window has w / W = 1).  u >= L3_r - the tail of a recording's last windows - gives +0.0f.
 * EVERY element of both outputs in [0, rec_win0[n_rec]) is written by the call, +0.0f where nothing above defines it; the
 * caller need not clear anything.  The gradient is that of the blended values as computed: the fp32 rounding of the blend
 * itself is not differentiated (every element within 5e-6 of its own magnitude + 1e-9 of the float64 central difference of
 * sum(g * weak): the bound tests/test_long_weak_bwd_cpu.py asserts).
 *   err  one int32, OR-ed (zero it first): a recording sed_stitch_weak rejects raises the same bits here (16 malformed
 *        tables - also a rec_frame0[n_rec] outside 1 .. 2^31 / NC - , 32 too few windows) and its windows are left zero.  A
 *        caller must treat all outputs as invalid when err != 0.  The address guarantee of sed_stitch_decode holds for all
 *        four window tensors.  Tables whose recordings share windows are not detected: the shared elements then hold one
 *        of the recordings' values.
 * Two launches on `stream`: a clear of both outputs (the window count is device data), then one tile pass - a workgroup
 * owns sed_stitch_tile_frames() frames of one recording, no halo; each timeline element blends both tensors once and
 * scatters to its <= ceil(T3 / hop3) covering windows; each window element has exactly one owner, so there are no atomics and
 * two calls give identical bytes.  16-byte accesses when NC % 4 == 0 and all four window tensors are 16-byte aligned, a
 * scalar path otherwise (identical bytes).  No workspace, no host synchronisation, no allocation, hipGraph-capturable.
 * Limits, checked before any launch (SED_ERR_BAD_ARG, outputs untouched): NC <= 16, 1 <= hop3 <= T3 <= 4096,
 * n_rec * NC < 2^31, no null pointer. */
int sed_stitch_weak_backward(const float* win_strong, const float* win_att, const int32_t* rec_win0,
                             const int64_t* rec_frame0, int n_rec, int T3, int NC, int hop3, int weighting,
                             const double* sums, const float* g_weak, float* d_win_strong, float* d_win_att,
                             int32_t* err, void* stream);

/* ---- span-level weak tags of long recordings, and a tag-gated decode --------------------------------
 * The recording-level tag says "class c occurs somewhere in recording r"; the span tags say it per span of span3 label frames,
 * and the gate lets them veto the strong decode the way task-4 systems mask a clip's strong posteriors with its weak
 * prediction.  The definitions are the project's own; pinned is agreement with a plain-loop statement (tests/span_tags_np.py).
 *
 * Spans.  span3 >= 1; recording r with L3_r timeline frames has S_r = ceil(L3_r / span3) spans, span s covers the frames
 * [s * span3, min((s + 1) * span3, L3_r)) - only the last may be shorter.  rec_span0 [n_rec + 1] int64 (device) holds the span
 * offsets: rec_span0[r + 1] - rec_span0[r] == S_r, total_spans = rec_span0[n_rec].
 *
 * Span tags.  P, A: the blends of win_strong / win_att exactly as for the recording-level tag above (one code; a frame covered
 * by one window is copied exactly).  For span g of recording r, class c, over the span's frames u, in fp64:
 *   num[g, c] = sum_u (double)P[u, c] * (double)A[u, c],  den[g, c] = sum_u (double)A[u, c],  tag[g, c] = (float)(num / den)
 * No special case for den == 0 or NaN inputs.
 *   tags [total_spans][NC] fp32;  sums [total_spans][NC][2] fp64 (num, den) or NULL
 * The order of the sums is a function of the span's length in frames and of NC alone - not of the span's position, its
 * recording, alignment or the 16-byte / scalar path - and it is the order the recording-level tag uses for a recording of that
 * length: the tile pass walks a span from ITS first frame with the recording-level tile body, the span pass is the
 * recording-level column pass.  A recording with one span (span3 >= L3_r) gets tags and sums bit-identical to the
 * recording-level ones; two spans of equal length over equal frames give equal bits.
 *   err  one int32, OR-ed (zero it first): 16 = malformed rec_win0 / rec_frame0 / rec_span0 - also a rec_span0 that disagrees
 *        with ceil(L3_r / span3) or reaches beyond total_spans - , 32 = a recording whose windows do not cover it.  Every tags /
 *        sums row in [0, total_spans) is written by the call: NaN where the row belongs to such a recording or to none, never
 *        stale.  (The recording of a row is found by bisection: a rec_span0 that is not increasing can moreover leave rows of a
 *        well-formed recording that the bisection assigns to another one; they are NaN too.)  The address guarantee of the
 *        stitched decode holds for both window tensors, the outputs and the workspace.
 *   ws   the _ws_bytes value for (sum L3, total_spans, n_rec, NC, span3), 8-byte aligned: one (num, den) pair per (tile slot,
 *        class), slot = span * ceil(span3 / tile frames) + k; ws_bytes must be that value
 * Two launches on `stream`, a tile pass and a span pass; no timeline is written, no float atomics, no host synchronisation, no
 * allocation, hipGraph-capturable.
 * Limits, checked before any launch (SED_ERR_BAD_ARG, outputs untouched): NC <= 16, 1 <= hop3 <= T3 <= 4096, span3 >= 1,
 * n_rec <= total_spans <= total_frames, total_frames * NC < 2^31, total_spans * NC < 2^31, tile slots < 2^31 (a caller clamps
 * an "infinite" span3 to the longest recording).
 *
 * Tag score of an event.  For event i = [on, off) of column (k, rec, c) of a CSR table (layout as for the event scores above):
 *   tag_score[i] = the largest non-NaN tags[rec_span0[rec] + s][c] over s = on / span3 .. (off - 1) / span3, NaN when every
 *   such tag is NaN: a copy of an input value, no arithmetic.  An event that ends on a span boundary does not touch the next
 *   span.  It is the event-score kernel's maximum under a coordinate map (rows = spans), one launch, flat over ev_pairs; the
 *   split between events reduced by their thread and by their wave is the event scores', applied to the spans touched.
 *   err  16 as for the event scores (columns; rec_span0 against total_spans), 64 = an event with on < 0, on >= off or
 *        off > S_rec * span3: its score is NaN and nothing of it is read.
 * Limits and overlap checks as for the event scores (total_spans * NC < 2^31 in the place of the frames), span3 >= 1.
 *
 * The gate.  An event is kept iff tag_score > min_tag[k][c]: strict, a NaN score is never kept.  That IS the select by score
 * above with key = 0 and the tag score in the score_max slot; there is no other kernel.  Consequences (tests pin them):
 *   1. with one span per recording a column is kept whole or dropped whole, exactly where the recording-level tag exceeds
 *      min_tag: the clip-level weak mask;
 *   2. an event that lies across a span boundary is kept when either side is confident;
 *   3. min_tag = -inf returns the table byte for byte;  4. a K-point call equals K one-point calls;
 *   5. the rule is "keep whole events that touch a confident span", NOT "zero the posteriors of unconfident spans, then
 *      decode", which cuts events at span boundaries.  By hand: span3 = 4, one class, tags (0.9, 0.1), min_tag 0.5, one
 *      decoded event [2, 7).  The gate keeps [2, 7) whole (it touches span 0); masking the posteriors of span 1 first and
 *      decoding would give [2, 4).
 *
 * Backward through the span tags: sed_stitch_span_tags_backward, the gradient of a loss on tags[g, c] w.r.t. both window
 * tensors.  It is sed_stitch_weak_backward's definition with ONE change: timeline frame u of recording r takes g, num and den
 * from row = rec_span0[r] + u / span3 of g_tags / sums, not from row r.  The same individually rounded fp64 operations in the
 * same order (t = num / den, dP = (g * A) / den, dA = (g * (P - t)) / den, outputs (float)((dP * w) / W), (float)((dA * w) / W)).
 *   sums   [total_spans][NC][2] fp64  the (num, den) pairs sed_stitch_span_tags returned for the same inputs
 *   g_tags [total_spans][NC]    fp32  dLoss/dtags
 * EVERY element of both outputs in [0, rec_win0[n_rec]) is written, +0.0f in the tails u >= L3_r and for rejected recordings.
 * Consequences (tests pin them): with one span per recording (span3 >= max L3, rec_span0 = 0 .. n_rec) the outputs are
 * byte-identical to sed_stitch_weak_backward's on the same sums; a span's gradient does not depend on the span's position,
 * its recording or the tiling; a g_tags row of zeros gives zeros (of either sign) on that span's frames.  The gradient is
 * that of the blended values as computed; against the float64 central difference an element is within
 * 5e-6 |fd| + 1e-9 + 2^-22 |g| (w / W) / den (tests/test_span_tags_bwd_cpu.py: a short span's den is small, and the fp32
 * rounding of the blended P and A enters dA absolutely).
 *   err  one int32, OR-ed (zero it first): 16 = malformed rec_win0 / rec_frame0 / rec_span0 - also a rec_span0 that disagrees
 *        with ceil(L3_r / span3) or reaches beyond total_spans, checked per recording in the clear pass - , 32 = a recording
 *        whose windows do not cover it.  Such a recording's windows are left +0.0f; no row outside [0, total_spans) is read.
 * Two launches on `stream` (clear, then the tile pass over the recordings' tiles: sed_stitch_weak_backward's two kernels with
 * the row lookup).  No atomics, no workspace, no host synchronisation, no allocation, hipGraph-capturable.  16-byte accesses
 * when NC % 4 == 0 and all four window tensors are 16-byte aligned, a scalar path otherwise (identical bytes).
 * Limits, checked before any launch (SED_ERR_BAD_ARG, outputs untouched): NC <= 16, 1 <= hop3 <= T3 <= 4096, span3 >= 1,
 * n_rec <= total_spans, total_spans * NC < 2^31, sums 8-byte aligned, no null pointer.
 *
 *
 * Span tags of PIECES: sed_stitch_piece_span_tags and sed_stitch_piece_span_tags_backward.  A span's tag depends only on the
 * windows that cover the span, so the spans of a recording with more windows than one forward holds can be pooled - and
 * trained on - in pieces: a piece is a run of consecutive spans plus exactly the windows that cover them.  The two entries are
 * the span entries with one more device table, rec_span_off [n_rec] int32, and a "recording" of the call is a piece.  It owns
 *   the windows rec_win0[r] .. rec_win0[r + 1], the local frames 0 .. L3_r from rec_frame0 (frame u of window j is local frame
 *   j * hop3 + u, as in a recording), and n_r = rec_span0[r + 1] - rec_span0[r] spans;
 *   span k of piece r covers the local frames [off_r + k * span3, min(off_r + (k + 1) * span3, L3_r)), off_r = rec_span_off[r].
 * A piece starts at a window boundary, not at a span boundary in general: the local frames below off_r and from
 * off_r + n_r * span3 on belong to no span.  Everything else is the definition above in the same code: the blend, the fp64 num /
 * den, tag = (float)(num / den), a tile walk that starts at the span's own first frame - so the order of a span's sums depends on
 * its length and NC alone, and a span pooled from a piece that holds all the windows covering it has the BITS the whole
 * recording's call gives it - and the backward's individually rounded fp64 operations in their order.  In the backward, frame
 * u of piece r reads row rec_span0[r] + (u - off_r) / span3; the window elements of a frame that belongs to no span are +0.0f
 * like the tails.  A piece's gradient is that of exactly the loss terms of its spans: over pieces that partition a recording's
 * spans, every window element is nonzero in at most one piece, and the element-wise sum is the whole call's gradient.
 *   err  16 also for a piece with off_r < 0, n_r < 1, off_r + (n_r - 1) * span3 >= L3_r (its last span would be empty) or a
 *        rec_span0 outside 0 .. total_spans, checked per piece before any value is used as an index; the rule
 *        n_r == ceil(L3_r / span3) of the span entries does NOT apply.  Such a piece's rows are NaN in the forward, its windows
 *        +0.0f in the backward; the other pieces are unaffected.  The address guarantee holds for every tensor whatever the
 *        tables contain.
 * With off = 0 and n_r = ceil(L3_r / span3) everywhere both entries return the span entries' bytes.  Launches, paths, workspace
 * (sed_stitch_piece_span_tags_ws_bytes: the span entry's value) and host-side limits are the span entries'.
 *
 * Not provided: overlapping or per-recording span lengths, masking in the frame domain. */
size_t sed_stitch_span_tags_ws_bytes(long long total_frames, long long total_spans, int n_rec, int nclass, int span3);
int sed_stitch_span_tags(const float* win_strong, const float* win_att, const int32_t* rec_win0, const int64_t* rec_frame0,
                         const int64_t* rec_span0, long long total_frames, long long total_spans, int n_rec, int T3, int NC,
                         int hop3, int weighting, int span3, float* tags, double* sums, void* ws, size_t ws_bytes, int32_t* err,
                         void* stream);
int sed_stitch_span_tags_backward(const float* win_strong, const float* win_att, const int32_t* rec_win0,
                                  const int64_t* rec_frame0, const int64_t* rec_span0, long long total_spans, int n_rec, int T3,
                                  int NC, int hop3, int weighting, int span3, const double* sums, const float* g_tags,
                                  float* d_win_strong, float* d_win_att, int32_t* err, void* stream);
size_t sed_stitch_piece_span_tags_ws_bytes(long long total_frames, long long total_spans, int n_rec, int nclass, int span3);
int sed_stitch_piece_span_tags(const float* win_strong, const float* win_att, const int32_t* rec_win0,
                               const int64_t* rec_frame0, const int64_t* rec_span0, long long total_frames,
                               long long total_spans, int n_rec, int T3, int NC, int hop3, int weighting, int span3,
                               const int32_t* rec_span_off, float* tags, double* sums, void* ws, size_t ws_bytes, int32_t* err,
                               void* stream);
int sed_stitch_piece_span_tags_backward(const float* win_strong, const float* win_att, const int32_t* rec_win0,
                                        const int64_t* rec_frame0, const int64_t* rec_span0, long long total_spans, int n_rec,
                                        int T3, int NC, int hop3, int weighting, int span3, const int32_t* rec_span_off,
                                        const double* sums, const float* g_tags, float* d_win_strong, float* d_win_att,
                                        int32_t* err, void* stream);
int sed_events_tag_scores(const float* tags, long long total_spans, const int64_t* rec_span0, int span3, int n_rec, int NC,
                          const int64_t* ev_ptr, const int32_t* ev_pairs, long long pairs_capacity, long long n_cols,
                          float* tag_score, int32_t* err, void* stream);

/* ---- pseudo strong labels: an event table rasterised into the rows of a label pool ------------------
 * The training side reads its strong labels as rows [*][NC] fp32 in HBM (the label pool the gather kernels slice); every
 * decode, gate, process and select leaves a CSR event table.  sed_events_rasterize turns a table back into label rows at
 * their place in such a pool, in place: the teacher's cleaned events become the next round's strong labels without a host
 * copy.  The definition is the project's own; pinned is bitwise agreement with a plain-loop statement
 * (tests/rasterize_np.py: for every recording, class and event, for u in range(on, off)).
 *   ev_ptr [n_points * n_rec * NC + 1] int64, ev_pairs [pairs_capacity][2] int32   a table in the sweep's column order
 *                                        (layout as for the event scores above; n_points = 1: sed_stitch_decode's)
 *   point [NC] int32                     device, or NULL for all zero: class c is taken from operating point point[c], its
 *                                        column is (point[c] * n_rec + rec) * NC + c - a tuned system keeps a point per class
 *   value [pairs_capacity] fp32          indexed like ev_pairs, or NULL: every event has the value 1.0f.  Otherwise the event's
 *                                        value is copied bit for bit (NaN payloads, -0.0f and denormals as they are);
 *                                        score_max / score_mean of sed_events_scores are the intended soft labels
 *   rec_frame0 [n_rec + 1] int64         device: recording r has L3_r = rec_frame0[r + 1] - rec_frame0[r] rows
 *   dst [dst_rows][NC] fp32              the pool
 *   dst_row0 [n_rec] int64               device, or NULL: row u of recording r is dst row dst_row0[r] + u; NULL means
 *                                        rec_frame0[r] + u, a contiguous timeline.  Exactly the L3_r rows of each valid
 *                                        recording are addressed; no other byte of dst is read or written.
 * For row u of recording r and class c: i = the event of the selected column with on_i <= u < off_i (columns hold disjoint
 * events with non-decreasing onsets: at most one), v = value[i] or 1.0f.
 *   combine = 0 (replace)  a covered element takes v, an uncovered one +0.0f: every addressed element is written exactly once
 *   combine = 1 (maximum)  a covered element takes (v > old) ? v : old - a NaN v never replaces anything, a NaN old stays - ,
 *                          an uncovered one is left as it is.  M calls form the union of M models' tables; one call on given
 *                          strong labels adds pseudo events to them.
 * Events are never cut except at L3_r, and an event beyond L3_r is an error, not a clip.
 *   err    one int32, OR-ed, the family's bits:
 *             8 = point[c] outside [0, n_points): class c is rasterised in no recording, its elements are not written
 *            16 = a column whose bounds are not 0 <= ev_ptr[col] <= ev_ptr[col + 1] <= pairs_capacity (any column of the
 *                 table, selected or not), a recording whose bounds are not 0 <= rec_frame0[r] <= rec_frame0[r + 1] <=
 *                 dst_rows (the rows of distinct destinations cannot number more than dst_rows), or a recording with
 *                 dst_row0[r] < 0 or dst_row0[r] + L3_r > dst_rows: nothing of such a column or recording is read or written.
 *                 (As in sed_events_hysteresis, an ev_ptr that is not non-decreasing can moreover leave events that the
 *                 bisection assigns to no column: they are not checked.)
 *                 (The recording of a row is found by bisection: a rec_frame0 that is not non-decreasing can moreover leave
 *                 rows of a well-formed recording that the bisection assigns to another one; they are not written.)
 *            64 = an event of a valid column that `point` selects, in a recording with valid frame bounds, with on < 0,
 *                 on >= off, off > L3_r, or on smaller than the previous event's off in the same column (touching events are
 *                 valid).  Every such event index is checked, not only those a row meets; what the column's elements hold
 *                 afterwards is unspecified (inside the addressed rows).
 *          No table content can make a kernel address outside ev_ptr, ev_pairs, value, point, rec_frame0, dst_row0 or the
 *          addressed rows of dst.  A caller treats dst as invalid when err != 0.  Two recordings whose destination rows overlap
 *          are a host error: the entry only guarantees in-bounds writes (the Python fronts refuse them).
 * Two launches on `stream` whatever n_points and the number of events are (one when dst_rows is 0): a check pass flat over
 * the indices of ev_pairs that writes nothing but err, and a row pass - a gather, flat over the timeline rows: a thread finds
 * its recording by bisection over rec_frame0 and per class the last event with on <= u by bisection over the column's
 * onsets.  The destination is not cleared first.  16-byte stores when NC % 4 == 0 and dst is 16-byte aligned, a scalar path
 * otherwise (identical bytes).  No workspace, no host synchronisation, no allocation, no atomics but the OR into err,
 * hipGraph-capturable, identical bytes from call to call.
 * Limits, checked before any launch (SED_ERR_BAD_ARG, err untouched): no null pointer except value, point and dst_row0,
 * 1 <= NC <= 16, n_rec >= 1, 1 <= n_points <= 4096, n_points * n_rec * NC < 2^26, 0 <= pairs_capacity < 2^31, 0 <= dst_rows,
 * dst_rows * NC < 2^31, ev_pairs 8-byte aligned, dst 4-byte aligned, combine 0 or 1, dst overlapping no input (err included).
 * Not provided: per-frame "ignore" labels, events cut at window or span boundaries, sub-frame onsets, feature pools. */
int sed_events_rasterize(const int64_t* ev_ptr, const int32_t* ev_pairs, const float* value, long long pairs_capacity,
                         int n_points, const int32_t* point, const int64_t* rec_frame0, int n_rec, int NC,
                         float* dst, long long dst_rows, const int64_t* dst_row0, int combine,
                         int32_t* err, void* stream);

/* ---- event-aware crop starts for windowed training, drawn from the label pool ------------------------
 * Uniform crop starts spend most windows of a sparsely labelled recording on silence.  These two entries draw the starts
 * of sed_gather_window_logmel_transform's windows from the label pool where it lives (since sed_events_rasterize the labels
 * that say where events are may exist in HBM only).  The definition is the project's own and uses integers only; pinned is
 * exact agreement with a plain-loop statement (tests/crop_np.py).
 *
 * Item i owns the R_i >= 1 label rows [label_row0[i], label_row0[i + 1]) of label_pool [total_label_rows][nclass] fp32
 * (label_row0: device int64 [n_items + 1], a CSR over the rows).  hi = start_hi[i] >= 0 is its last legal start, T3 the
 * window length in label frames.  A row is ACTIVE for class c when label_pool[row][c] > 0 (NaN, -0.0f and anything <= 0 are
 * inactive, a soft label counts as active).
 *   a_c(s)  = active rows of class c in [s, min(s + T3, R))             C_c(s) = sum of a_c(s') over s' <= s, s in [0, hi]
 *   W_c     = C_c(hi); class c is PRESENT in the item when W_c > 0;     P = the number of present classes
 * All randomness is the caller's: per window slot u (uint64, uniform on [0, 2^64)), v (int32 >= 0) and m (uint8).
 *   m == 0 or P == 0:  start = (u * (hi + 1)) >> 64  (the high 64 bits of the 64 x 64 bit product), chosen class -1
 *   otherwise:         c = the (v % P)-th present class in class order, target = (u * W_c) >> 64,
 *                      start = the smallest s with C_c(s) > target
 * so a_c(start) > 0 - the window holds an active frame of c - and a start's probability is proportional to the activity of
 * c its window covers.
 *
 * sed_window_activity: one segmented scan over the pool, flat over rows, of the triples (n, a, b) under
 *   (n1, a1, b1) o (n2, a2, b2) = (n1 + n2, a1 + a2, b1 + b2 + a1 * n2), reset at every item's first row.  In front of row x
 * of an item it leaves A(x) = the active rows before x and B(x) = A(0) + ... + A(x - 1), for x in [0, R]:
 *   A [(total_label_rows + n_items)][nclass] int32, B likewise int64: item i's R_i + 1 rows start at row label_row0[i] + i.
 * Beyond R both are extended on read, A(x) = A(R) and B(x) = B(R) + (x - R) * A(R); then
 *   C_c(s) = B(s + 1 + T3) - B(T3) - B(s + 1).
 *   W [n_items][nclass] int64, present [n_items] uint32 (bit c: W_c > 0): written from three reads of B per class.
 *   ws = sed_window_activity_ws_bytes(total_label_rows, n_items, nclass) bytes, 8-byte aligned (0 and sed_last_error for
 *   sizes outside the limits below).
 * Four launches on `stream` whatever the items' lengths are: the reduction of every tile of 256 rows, a one-workgroup scan
 * of the tiles' reductions, the tiles' scans behind their carries, and a thread per item for W and present.  No item is
 * walked by one thread or one workgroup.  Wave steps are shuffles, waves meet in LDS; integer arithmetic only, so the
 * bytes do not depend on the geometry.
 *
 * sed_window_event_starts: one thread per slot j < n_slots reads u[j], v[j], m[j], i = slot_item[j] (int32), start_hi[i] and
 * the tables above, and writes start3[j] and chosen[j] (int32 each; chosen = -1 for a uniform draw).  The start is found by
 * bisection of C_c over [0, hi]: it lies in [0, hi] whatever the tables hold.  One launch (none for n_slots == 0).
 *
 *   err    one int32, OR-ed, the family's bits:
 *             8 = nclass > 16 (the mask's width): one launch that raises the bit; nothing else is read or written
 *            16 = an item whose rows are not 0 <= label_row0[i] < label_row0[i + 1] <= total_label_rows: neither its W /
 *                 present (activity) nor a slot that names it (starts) is written; a slot_item outside [0, n_items): that
 *                 slot is not written.  (The item of a row is found by bisection: a label_row0 that is not non-decreasing can
 *                 moreover leave rows that the bisection assigns to no valid item; they are neither read nor written.)
 *            32 = start_hi[i] < 0 (activity: the item's W / present are not written), or in sed_window_event_starts
 *                 start_hi[i] < 0 or start_hi[i] * pool_ratio >= clip_frames[i] - a start the gather's caller would refuse:
 *                 the slot is not written
 *          No table content can make a kernel address outside its arguments.  A caller treats the outputs as invalid when
 *          err != 0.
 * No host synchronisation, no allocation, no atomics but the OR into err, hipGraph-capturable, identical bytes from call to
 * call.  Limits, checked before any launch (SED_ERR_BAD_ARG, err untouched; SED_ERR_WORKSPACE for a ws_bytes that is not the
 * size function's value): no null pointer, 1 <= total_label_rows < 2^31, 1 <= n_items < 2^26, nclass >= 1, T3 >= 1,
 * pool_ratio >= 1, 0 <= n_slots < 2^31, u, B, W and ws 8-byte aligned.
 * Not provided: class balance across items, weights from event scores, starts finer than a label frame.               */
size_t sed_window_activity_ws_bytes(long long total_label_rows, int n_items, int nclass);
int sed_window_activity(const float* label_pool, const int64_t* label_row0, long long total_label_rows, int n_items,
                        int nclass, const int32_t* start_hi, int T3, int32_t* A, int64_t* B, int64_t* W,
                        uint32_t* present, void* ws, size_t ws_bytes, int32_t* err, void* stream);
int sed_window_event_starts(const uint64_t* u, const int32_t* v, const uint8_t* m, const int32_t* slot_item,
                            long long n_slots, const int32_t* start_hi, const int32_t* clip_frames, int pool_ratio,
                            const int64_t* label_row0, long long total_label_rows, int n_items, int nclass, int T3,
                            const int32_t* A, const int64_t* B, const int64_t* W, const uint32_t* present,
                            int32_t* start3, int32_t* chosen, int32_t* err, void* stream);

/* ---- validation scoring ------------------------------------------------------------------------
 * Replaces, after get_predictions, the host-side scoring of the epoch loop (baseline/main.py:328-352):
 *   compute_strong_metrics(predictions, valid_synth_df) (evaluation_measures.py:234-246) = sed_eval's
 *   EventBasedMetrics(t_collar = 0.2, percentage_of_length = 0.2, 'zero_score', optimal matching) and
 *   SegmentBasedMetrics(time_resolution = 1) fed per file (evaluation_measures.py:124-182), and
 *   get_f_measure_by_class / intermediate_at_measures (evaluation_measures.py:19-102).
 * sed_eval is third-party, absent from this image and from the reference tree: the event / segment definitions
 * are restated from its published algorithm - parity with sed_eval itself is UNPINNED (as for dcase_util in
 * sed_postprocess); pinned is exact agreement with an independent numpy / scipy statement of the definitions
 * (tests/sed_eval_np.py).
 *
 * sed_event_counts, per (operating point k, clip, class) column:
 *   estimated events: strong != NULL: threshold thr[k] -> median filter win[k] (1 .. 63) -> run-length decode exactly
 *     as sed_postprocess, seconds = (double)frame * num / den (num = pooling_time_ratio, den = sample_rate /
 *     hop_length: the host's doubles bit for bit); strong == NULL: given as est_ptr / est_on / est_off (CSR like
 *     the reference events, n_points = 1, need not be disjoint).
 *   reference events: ref_ptr [n_clips * nclass + 1] int32 offsets into ref_on / ref_off (fp64 seconds), column
 *     (clip, class) = clip * nclass + class.
 *   event-based: r and e are compatible iff |r.on - e.on| <= t_collar and |r.off - e.off| <= max(t_collar,
 *     percentage_of_length * (r.off - r.on)); Ntp = size of a MAXIMUM bipartite matching; Nref, Nsys = list lengths.
 *   segment-based: an event covers segments max(0, floor(on / res)) .. ceil(off / res) - 1; the file has
 *     ceil(max offset over both lists and all classes / res) segments; Ntp, Nfp, Nfn, Ntn per class.
 *   ev_counts  [n_points][n_clips][nclass][3] int32 (Ntp, Nref, Nsys) or NULL
 *   seg_counts [n_points][n_clips][nclass][4] int32 (Ntp, Nfp, Nfn, Ntn) or NULL
 *   ev_total   [n_points][nclass][3], seg_total [n_points][nclass][4] int64: ACCUMULATED over clips (zero them
 *              before the first batch; integer sums: bit-reproducible)
 *   err        one int32, OR-ed: 1 = a column with more than 64 reference events, 2 = more than 64 estimated
 *              events, 4 = a file of more than 65 536 segments, 8 = a window outside 1 .. 63, 16 = malformed
 *              offsets.  Such a column is not scored (never a truncated count): a caller must treat the totals as
 *              invalid when err != 0.
 * Limits: T <= 2048, nclass <= 16 (the scoring limits and the err bits are defined once, in csrc/score.h, for
 * these calls and the sed_long_* ones).  The overall error rate with substitutions (a second, label-agnostic
 * matching) comes from sed_error_counts ("overall error rate", below).
 * sed_weak_counts: weak [n_clips][nclass] fp32, labels [n_clips][nclass] uint8, thr [n_points][nclass] ->
 *   counts [n_points][nclass][4] int64 (tp, fp, fn, tn) with pred = weak > thr, ACCUMULATED (chain the batches).
 * Both: one launch on `stream`, no allocation, hipGraph-capturable. */
int sed_event_counts(const float* strong, int n_clips, int T, int nclass, int n_points, const float* thr,
                     const int32_t* win, double num, double den, const int32_t* est_ptr, const double* est_on,
                     const double* est_off, const int32_t* ref_ptr, const double* ref_on, const double* ref_off,
                     double t_collar, double percentage_of_length, double time_resolution, int32_t* ev_counts,
                     int32_t* seg_counts, int64_t* ev_total, int64_t* seg_total, int32_t* err, void* stream);
int sed_weak_counts(const float* weak, const uint8_t* labels, int n_clips, int nclass, const float* thr,
                    int n_points, int64_t* counts, void* stream);

/* ---- PSDS intersection counts ------------------------------------------------------------------
 * The polyphonic sound detection score (Bilen et al., ICASSP 2020) is the area under a PSD-ROC built from a grid of
 * operating points, each scored with three intersection criteria.  sed_psds_counts produces the integer counts of
 * every operating point in one launch; the curve and its area are host arithmetic (metrics.PSDS).
 * psds_eval is third-party, absent from this image and from the reference tree: the definitions below are restated
 * from the paper, and where the package's behaviour was uncertain the text below decides - parity with psds_eval
 * itself is UNPINNED (as for sed_eval above); pinned is exact agreement with an independent numpy statement of
 * these definitions (tests/psds_np.py).
 *
 * Per (operating point k, clip); classes are columns; an event is (on, off) in fp64 seconds.  Detections: decoded
 * from `strong` exactly as sed_event_counts does (thr[k], win[k], seconds = (double)frame * num / den), or given as
 * est_ptr / est_on / est_off (strong == NULL, n_points = 1).  Ground truths: ref_ptr / ref_on / ref_off as above,
 * in stored order.
 *   I(d, g) = max(0, min(d.off, g.off) - max(d.on, g.on));  len(e) = e.off - e.on.
 *   Every sum is a sequential fp64 sum over the other side's events in stored index order, starting from 0.0; every
 *   test is sum / len >= threshold (the division first); an event with len <= 0, or a NaN ratio, fails every test.
 *   DTC:  detection d of class c is RELEVANT iff (sum over g in G_c of I(d, g)) / len(d) >= dtc.
 *         FP[c] = detections of c that are not relevant (those that turn out to be cross-triggers included).
 *   GTC:  ground truth g of class c is a true positive iff (sum over the RELEVANT d in D_c of I(d, g)) / len(g) >= gtc.
 *         TP[c] = their number.
 *   CTTC: for every non-relevant detection d of class c and every other class j: CT[c][j] += 1 iff
 *         (sum over g in G_j of I(d, g)) / len(d) >= cttc.  CT[c][c] = 0.
 *   dtc, gtc, cttc in [0, 1] (the task's values: 0.5, 0.5, 0.3).
 *   columns    [n_points][n_clips][nclass][2 + nclass] int32 (TP, FP, CT[.][0 .. nclass - 1]) or NULL
 *   totals     [n_points][nclass][2 + nclass] int64: ACCUMULATED over clips (zero them before the first batch;
 *              integer sums: bit-reproducible)
 *   err        the error word of sed_event_counts, same bits (1, 2: more than 64 reference / estimated events in a
 *              column, 8: a window outside 1 .. 63, 16: malformed offsets; 4 is never raised here).  Nothing is
 *              truncated: a caller must treat the totals as invalid when err != 0.
 * Limits: T <= 2048, nclass <= 16.  One launch on `stream`, no allocation, hipGraph-capturable. */
int sed_psds_counts(const float* strong, int n_clips, int T, int nclass, int n_points, const float* thr,
                    const int32_t* win, double num, double den, const int32_t* est_ptr, const double* est_on,
                    const double* est_off, const int32_t* ref_ptr, const double* ref_on, const double* ref_off,
                    double dtc, double gtc, double cttc, int32_t* columns, int64_t* totals, int32_t* err,
                    void* stream);

/* ---- scoring long recordings -------------------------------------------------------------------
 * sed_long_event_counts / sed_long_psds_counts score the event table sed_stitch_decode leaves (or events given in
 * seconds) against reference events, for (recording, class) columns of ANY length.  The definitions are those of
 * sed_event_counts and sed_psds_counts above - compatibility and Ntp = size of a maximum bipartite matching; segment
 * coverage, the file's segment count and the four segment counts; DTC / GTC / CTTC with every sum a sequential fp64
 * sum in stored order from 0.0 and the division first - with ONE exception: there is no limit of 64 events per column.
 * Pinned: exact agreement with tests/sed_eval_np.py and tests/psds_np.py, which state the definitions for lists of any
 * length; parity with sed_eval / psds_eval stays UNPINNED as above.
 *
 * Columns are (recording, class) = rec * nclass + class.  One operating point per call (K points: the sweep calls below).
 *   estimated events  ev_ptr [n_rec * nclass + 1] int64 CSR offsets, and either
 *                     ev_pairs [est_capacity][2] int32 (onset, exclusive offset) frames as sed_stitch_decode writes them:
 *                       seconds = (double)frame * num / den, the host's doubles bit for bit (est_on / est_off ignored), or
 *                     ev_pairs == NULL and est_on / est_off [est_capacity] fp64 seconds (they need not be disjoint)
 *   reference events  ref_ptr [n_rec * nclass + 1] int64, ref_on / ref_off [ref_events] fp64 seconds
 *   est_capacity, ref_events   what the arrays hold (the capacity sed_stitch_decode was given, not the true count): every
 *                     offset is checked against them before it is used, and they size the grids and the workspace - all
 *                     known on the host without a synchronisation
 * BOTH SIDES OF A COLUMN MUST BE SORTED BY ONSET, non-decreasing (sed_stitch_decode's tables and arrays packed by
 * (onset, offset) are).  It is checked on the device: a column whose onsets decrease raises bit 64 and is not scored.
 * Two consequences of the order carry the long columns:
 *  1. The matching decomposes at valid cuts.  Merge the two onset lists of a column (ties in any order).  A cut after
 *     merged position p is VALID iff (last reference onset at or before p) + t_collar < (first estimated onset after p)
 *     and (last estimated onset at or before p) + t_collar < (first reference onset after p); a missing side counts as
 *     minus / plus infinity.  No compatible pair straddles a valid cut, so Ntp of the column is the sum of Ntp over the
 *     CLUSTERS, the maximal runs between valid cuts, and each cluster is matched exactly (the augmenting-path search
 *     of sed_event_counts).  The kernel evaluates "a + t_collar < b" as "b - a > t_collar", the form the compatibility
 *     test itself uses, so that no pair that test accepts can straddle a cut whatever the rounding; the two forms agree
 *     whenever the sum is exact.
 *     A cluster with more than 64 reference events raises bit 1, with more than 64 estimated events bit 2: events
 *     whose onsets chain within t_collar.  Such a column is not scored and nothing is truncated.  Estimated events
 *     between two clusters and reference events without a neighbour are clusters of their own: a column of thousands
 *     of events raises nothing as long as no single chain exceeds 64 per side.
 *  2. The PSDS sums skip zero terms.  Every I(d, g) >= 0 and the sum starts at 0.0, so leaving out events that do not
 *     overlap gives the bits of the full sequential sum; the kernels restrict each sum to the range of the other side
 *     that can overlap (still in stored order) and never visit every pair.
 * sed_long_event_counts outputs:
 *   ev_counts  [n_rec][nclass][3] int32 (Ntp, Nref, Nsys) or NULL;  seg_counts [n_rec][nclass][4] int32 (Ntp, Nfp, Nfn,
 *   Ntn) or NULL: every element is written (a column that is not scored: Ntp = 0 and four zeros)
 *   ev_total [nclass][3], seg_total [nclass][4] int64: ACCUMULATED over calls (zero them first)
 *   err  one int32, OR-ed: 1 / 2 = a cluster of more than 64 reference / estimated events, 4 = a recording of more than
 *        65 536 segments, 16 = malformed offsets (negative, decreasing or beyond est_capacity / ref_events), 64 = a
 *        column whose onsets decrease.  A caller must treat the totals as invalid when err != 0.
 * sed_long_psds_counts outputs: columns [n_rec][nclass][2 + nclass] int32 or NULL, totals [nclass][2 + nclass] int64
 *   ACCUMULATED, err with bits 16 and 64 only (no matching: 1 and 2 cannot be raised, 4 is not either).
 * ws: sed_long_score_ws_bytes(est_capacity, ref_events, n_rec, nclass) bytes, 8-byte aligned, for either call: the
 *   seconds of the frames, the running maxima of the offsets, per-column counters.
 * The matching is split along a column: one wave owns sed_long_tile_events() consecutive reference events, finds the
 *   clusters that start among them by a local test (two bisections per event) and follows the last one into the next
 *   tile.  Segments: one thread per segment.  PSDS: one thread per event.  Data passes between workgroups only from one
 *   launch to the next (four launches per call on `stream`).  No allocation, no host synchronisation, no float atomics;
 *   integer results are bit-reproducible; hipGraph-capturable.  No table content can make a kernel address outside the
 *   arrays as est_capacity / ref_events and n_rec * nclass + 1 describe them.
 * Limits: nclass <= 16, est_capacity and ref_events < 2^31 - 1024, n_rec * nclass < 2^26.  Not provided: an exact
 *   matching for clusters beyond 64 per side.  The overall error rate with substitutions comes from
 *   sed_long_error_counts / sed_long_sweep_error_counts ("overall error rate", below).  Recording-level weak tags come
 *   from sed_stitch_weak and are scored by sed_weak_counts. */
size_t sed_long_score_ws_bytes(long long est_capacity, long long ref_events, int n_rec, int nclass);
int sed_long_tile_events(void);
int sed_long_event_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den, const double* est_on,
                          const double* est_off, long long est_capacity, const int64_t* ref_ptr, const double* ref_on,
                          const double* ref_off, long long ref_events, int n_rec, int nclass, double t_collar,
                          double percentage_of_length, double time_resolution, int32_t* ev_counts, int32_t* seg_counts,
                          int64_t* ev_total, int64_t* seg_total, int32_t* err, void* ws, size_t ws_bytes, void* stream);
int sed_long_psds_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den, const double* est_on,
                         const double* est_off, long long est_capacity, const int64_t* ref_ptr, const double* ref_on,
                         const double* ref_off, long long ref_events, int n_rec, int nclass, double dtc, double gtc,
                         double cttc, int32_t* columns, int64_t* totals, int32_t* err, void* ws, size_t ws_bytes,
                         void* stream);

/* ---- scoring K operating points of long recordings ---------------------------------------------
 * sed_long_sweep_event_counts / sed_long_sweep_psds_counts are the two calls above for n_points = K estimated tables
 * against ONE reference side.  The definitions are exactly those of the one-point calls (clusters between valid cuts,
 * an exact matching per cluster of at most 64 events per side, segments, DTC / GTC / CTTC with sequential fp64 sums in
 * stored order); pinned is byte-for-byte agreement with K one-point calls.
 *   estimated side    the table of sed_stitch_sweep: ev_ptr [K * n_rec * nclass + 1] int64, column (k, rec, c) =
 *                     (k * n_rec + rec) * nclass + c, with ev_pairs [est_capacity][2] frames, or ev_pairs == NULL and
 *                     est_on / est_off [est_capacity] fp64 seconds in the same column order
 *   reference side    unchanged: ref_ptr [n_rec * nclass + 1], shared by all points; estimated column (k, rec, c) is
 *                     scored against reference column (rec, c)
 *   The recording-level quantities are (k, rec)-level: the segment count of a file is taken over the reference events
 *   and point k's estimated events only.
 *   ev_counts [K][n_rec][nclass][3], seg_counts [K][n_rec][nclass][4], columns [K][n_rec][nclass][2 + nclass] int32 or
 *   NULL (every element is written); ev_total [K][nclass][3], seg_total [K][nclass][4], totals [K][nclass][2 + nclass]
 *   int64, ACCUMULATED over calls.  err: the bits of the one-point calls; a column that is not scored stays unscored in
 *   its own point only (a reference column that is not scored is unscored at every point).
 * Four launches per call whatever K is.  Everything that derives from the reference alone - the validation of its
 * offsets, the order check, the running maxima of its offsets - is done once per call, not once per point.
 * ws: sed_long_sweep_ws_bytes(est_capacity, ref_events, n_rec, nclass, K) bytes, 8-byte aligned.
 * The guarantees are those of the one-point calls.  Limits: 1 <= K <= 4096, K * n_rec * nclass < 2^26, est_capacity
 * (all points together) and ref_events < 2^31 - 1024, K * (ref_events / sed_long_tile_events() + n_rec * nclass + 1) < 2^31. */
size_t sed_long_sweep_ws_bytes(long long est_capacity, long long ref_events, int n_rec, int nclass, int n_points);
int sed_long_sweep_event_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den,
                                const double* est_on, const double* est_off, long long est_capacity,
                                const int64_t* ref_ptr, const double* ref_on, const double* ref_off, long long ref_events,
                                int n_rec, int nclass, int n_points, double t_collar, double percentage_of_length,
                                double time_resolution, int32_t* ev_counts, int32_t* seg_counts, int64_t* ev_total,
                                int64_t* seg_total, int32_t* err, void* ws, size_t ws_bytes, void* stream);
int sed_long_sweep_psds_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den,
                               const double* est_on, const double* est_off, long long est_capacity,
                               const int64_t* ref_ptr, const double* ref_on, const double* ref_off, long long ref_events,
                               int n_rec, int nclass, int n_points, double dtc, double gtc, double cttc, int32_t* columns,
                               int64_t* totals, int32_t* err, void* ws, size_t ws_bytes, void* stream);

/* ---- overall error rate -------------------------------------------------------------------------
 * The headline of both sed_eval reports is the OVERALL error rate, ER = (S + D + I) / Nref, in which an error of one
 * class against an error of another class counts once, as a substitution.  sed_error_counts, sed_long_error_counts and
 * sed_long_sweep_error_counts produce its integer counts per file (clip / recording; per (point, recording) in a sweep)
 * beside the class-wise calls above; the rates are host arithmetic (metrics.EventMetrics / SegmentMetrics, overall=).
 *
 * Segment-based (sed_eval's, exactly).  Segment cover and the file's segment count are those of sed_event_counts.  For
 * segment s let R_s / E_s be the set of classes with a reference / estimated event covering s, fn_s = |R_s \ E_s|,
 * fp_s = |E_s \ R_s|:   S += min(fn_s, fp_s),  D += max(0, fn_s - fp_s),  I += max(0, fp_s - fn_s).
 *   ER = (S + D + I) / Nref with Nref = sum over classes of (Ntp_c + Nfn_c) of seg_total.  Against seg_total of the same
 *   inputs:  S + D = sum_c Nfn_c  and  S + I = sum_c Nfp_c.
 * Event-based.  r and e are TIME-COMPATIBLE iff the compatibility test of sed_event_counts holds with the label ignored:
 *   |r.on - e.on| <= t_collar and |r.off - e.off| <= max(t_collar, percentage_of_length * (r.off - r.on)).
 *   Nany = size of a MAXIMUM bipartite matching over ALL events of the file under time-compatibility.  With Ntp = sum_c
 *   Ntp_c of the label-wise matching (ev_total), Nref and Nsys the numbers of events of all classes:
 *     Nsubs = Nany - Ntp,  Nfn = Nref - Nany,  Nfp = Nsys - Nany,  ER = (Nsubs + Nfn + Nfp) / Nref.
 *   Every same-label matching is a time-compatible matching, so Ntp <= Nany <= min(Nref, Nsys).
 *   THIS IS A DECISION.  sed_eval finds substitutions by a greedy pass over the events its label-wise matching left over;
 *   that count depends on the order of the lists and on WHICH maximum matching its matcher returned, so it is not a function
 *   of the two event sets and cannot be pinned.  Label-wise matching plus greedy substitutions is itself a time-compatible
 *   matching: sed_eval's Nsubs is never larger than this one and its ER never smaller, and the two agree whenever the
 *   greedy pass is itself maximum.  Parity with sed_eval stays UNPINNED, as for the rest of the section; pinned is exact
 *   agreement with tests/error_rate_np.py (sets per segment; scipy's matching on the double-loop matrix).
 *
 * sed_error_counts: the arguments of sed_event_counts up to time_resolution (posteriors decoded at n_points operating
 *   points, or given events), then
 *   ev_overall        [n_points][n_clips][3] int32 (Nref, Nsys, Nany) or NULL
 *   seg_overall       [n_points][n_clips][3] int32 (S, D, I) or NULL
 *   ev_overall_total  [n_points][3], seg_overall_total [n_points][3] int64, ACCUMULATED over clips (zero them first)
 *   err               the error word of sed_event_counts, same bits.  The clip's events of all classes are merged by onset
 *                     per side and cut into clusters by the valid-cut rule of the long calls above, applied to the MERGED
 *                     lists; each cluster is matched exactly.  More than 64 events per side in one merged cluster raises
 *                     bit 1 / 2 (as does a single column beyond 64); the clip is then not scored (Nany = S = D = I = 0,
 *                     Nref and Nsys as they are) and nothing is truncated.
 *   One launch: one workgroup per (point, clip), all class columns decoded into LDS as for sed_psds_counts.
 * sed_long_error_counts / sed_long_sweep_error_counts: the arguments of sed_long_event_counts /
 *   sed_long_sweep_event_counts (both sides of every class column sorted by onset), outputs ev_overall / seg_overall
 *   [n_rec][3] ([K][n_rec][3]) int32 or NULL (every element is written), the totals [3] ([K][3]) int64 ACCUMULATED, err
 *   with the bits of sed_long_event_counts (1 / 2: a MERGED cluster beyond 64 per side; 64: a class column whose onsets
 *   decrease - a recording with any such column is not scored).  ws: sed_long_error_ws_bytes / sed_long_sweep_error_ws_bytes
 *   bytes, 8-byte aligned (the workspace of the class-wise call plus the merged tables).
 *   Per recording and side the onset-sorted union of the class columns is built in the workspace - an event's rank is its
 *   index in its own column plus one bisection count per other column, ties by (class, index): no atomics, one writer per
 *   slot - and the cluster / tile matching of sed_long_event_counts runs on it as a one-class problem.  The reference side
 *   is validated and merged once per call, not once per point.  Segments: one thread per segment, a 16-bit class mask per
 *   side.  Six launches whatever K is.
 * All three share the guarantees of the calls they sit beside: no allocation, no host synchronisation, no float atomics,
 * integer bit-reproducible results, hipGraph-capturable; no table content can make a kernel address outside its arrays.
 * Not provided: sed_eval's order-dependent greedy count, an exact matching for merged clusters beyond 64 per side,
 * substitutions per class pair, error rates of the weak tags. */
int sed_error_counts(const float* strong, int n_clips, int T, int nclass, int n_points, const float* thr,
                     const int32_t* win, double num, double den, const int32_t* est_ptr, const double* est_on,
                     const double* est_off, const int32_t* ref_ptr, const double* ref_on, const double* ref_off,
                     double t_collar, double percentage_of_length, double time_resolution, int32_t* ev_overall,
                     int32_t* seg_overall, int64_t* ev_overall_total, int64_t* seg_overall_total, int32_t* err,
                     void* stream);
size_t sed_long_error_ws_bytes(long long est_capacity, long long ref_events, int n_rec, int nclass);
size_t sed_long_sweep_error_ws_bytes(long long est_capacity, long long ref_events, int n_rec, int nclass, int n_points);
int sed_long_error_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den, const double* est_on,
                          const double* est_off, long long est_capacity, const int64_t* ref_ptr, const double* ref_on,
                          const double* ref_off, long long ref_events, int n_rec, int nclass, double t_collar,
                          double percentage_of_length, double time_resolution, int32_t* ev_overall, int32_t* seg_overall,
                          int64_t* ev_overall_total, int64_t* seg_overall_total, int32_t* err, void* ws, size_t ws_bytes,
                          void* stream);
int sed_long_sweep_error_counts(const int64_t* ev_ptr, const int32_t* ev_pairs, double num, double den,
                                const double* est_on, const double* est_off, long long est_capacity,
                                const int64_t* ref_ptr, const double* ref_on, const double* ref_off, long long ref_events,
                                int n_rec, int nclass, int n_points, double t_collar, double percentage_of_length,
                                double time_resolution, int32_t* ev_overall, int32_t* seg_overall,
                                int64_t* ev_overall_total, int64_t* seg_overall_total, int32_t* err, void* ws,
                                size_t ws_bytes, void* stream);

/* ---- single-kernel replay (measurement) ----------------------------------------------------
 * Re-launches ONE kernel of the step on the buffers left by a finished sed_crnn_forward +
 * sed_crnn_backward (same shapes, same data; outputs are rewritten with identical values), so
 * that a caller can bracket it with HIP events on `stream` (bench.py's roofline leg) and so that
 * tests can exercise one kernel at a time.  name is one of
 *   "x_moments" "blk0_fwd" "conv1_fwd" "glu1_fwd" "conv2_fwd" "glu2_fwd" "gru0_fwd" "gru1_fwd" "heads_fwd"
 *   "gru1_bwd" "gru0_bwd" "gru_wgrad" "glu2_bwd" "conv2_wgrad" "conv2_dgrad" "glu1_bwd" "conv1_wgrad" "conv1_dgrad" "blk0_bwd"
 *   (the heads backward needs the loss inputs and is not replayable on its own). */
int sed_kernel_replay(const char* name, const sed_dims* d, const float* params, const float* x,
                      const uint64_t* seed_dev, void* ctx, size_t ctx_bytes, float* grads, void* ws,
                      size_t ws_bytes, void* stream);

/* Debug knob (returns the previous value); 0 = normal operation.  Each bit selects the second implementation a test
 * compares against, or a measurement aid.  Every other bit is ignored: the A/B variants that earlier rounds kept behind
 * them were removed. */
#define SED_DEBUG_DIRECT_CONV    (1 << 6)   /* fp32 64 -> 64 convolutions (forward, dgrad) by the direct 9-tap kernels, not Winograd F(2x2, 3x3) */
#define SED_DEBUG_DIRECT_WGRAD   (1 << 7)   /* fp32 64 -> 64 conv weight gradients by the direct kernels (k_wgrad16_db, k_conv3x3_wgrad<4, 3>) */
#define SED_DEBUG_STFT_R2        (1 << 19)  /* log-mel front end by round 2's kernel k_stft_mel (one workgroup per frame) */
#define SED_DEBUG_STFT_R3        (1 << 21)  /* log-mel front end by round 3's kernel k_stft_mel16 (one wave per frame) */
#define SED_DEBUG_SEPARATE_HEADS (1 << 24)  /* sed_mt_step_backward: the deferred heads by k_heads_fwd / k_heads_bwd, not fused into the backward recurrence */
#define SED_DEBUG_SLAB_WGRAD     (1 << 26)  /* fp32 block-2 (W = 4) weight gradient by k_wgrad_wino<4> (one partial slab per tile), not k_wgrad4_os */
#define SED_DEBUG_STRICT_F32     (1 << 27)  /* strict fp32: no split-bf16 products anywhere in the step */
#define SED_DEBUG_NO_SIDE_STREAM (1 << 30)  /* no helper stream: every kernel on the caller's stream (near-solo kernel times) */
int sed_debug_set(int flags);
/* Always 1: the direct kernels behind SED_DEBUG_DIRECT_CONV / SED_DEBUG_DIRECT_WGRAD are part of every build. */
int sed_build_flags(void);

/* ---- self tests (run on the GPU box by tests/) ---------------------------------------------
 * Checks the MFMA fragment mapping and Philox stream this build assumes. out[0..3] receives
 * max abs errors / mismatch counts; returns 0 if all checks pass. */
int sed_selftest(float* out_dev4, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DCASE_SED_H */

// rnn.h - the recurrent tail shared by the two orchestrators (rnn.hip): BiGRU + output heads, forward and backward, for
// H = 64 (gru4.hip) and H = 256 (ggemm.hip + grec.hip / ggru.hip), and the handle of the backward's helper stream; internal.
#pragma once
#include "common.h"
#include "kernels.h"

// ---- helper stream of one backward call ------------------------------------------------------------------------------------
// The dX chain (heads -> GRU -> dgrad2 -> dgrad1 -> block 0) is serial; the GRU dW / db GEMMs and the conv wgrads only feed
// the optimiser.  They are forked onto the helper stream of the caller's stream (crnn.hip: SideStream) and joined before the
// call returns, so the caller still sees one stream-ordered op and a hipGraph capture records the fork / join as graph edges.
// A fork has two halves, and the kernel of the critical chain goes BETWEEN them:
//     side.mark(st);  <launch on st>;  side.start();  <launches on side.s>
// Both kernels depend on the same event, but the one on st is CAPTURED FIRST.  The graph executor keeps the first-captured child
// of a node on its parent's hardware queue, and a replayed hipGraph serialises nodes that share a queue in creation order.
// With the helper stream's kernel captured first
//   - conv dgrad2 hopped to another queue and started 10 us late (profiles/r05b_mt-f32_step_timeline.txt: 447.6 -> 457.7 us);
//   - the 145 us wgrad kernel sat in front of dgrad1 + block 0 on one queue (profiles/r03_a_wide-bf16_step_timeline.txt);
//   - the H = 256 dX GEMM paid ~10 us of cross-queue latency per layer (profiles/r05b_wide-bf16_step_timeline.txt: "idle 9.9").
struct SideFork {
    hipStream_t s = nullptr;                     // where the forked work goes: the helper stream, or the caller's own when !ok
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool ok = false;                             // a helper stream exists and SED_DEBUG_NO_SIDE_STREAM is clear
    bool forked = false;                         // s carries work that join() has to wait for
    int mark(hipStream_t st) { if (ok) SED_CHECK_HIP(hipEventRecord(ev_fork, st)); return SED_OK; }
    int start() { if (ok) { SED_CHECK_HIP(hipStreamWaitEvent(s, ev_fork, 0)); forked = true; } return SED_OK; }
    int join(hipStream_t st) {
        if (forked) { SED_CHECK_HIP(hipEventRecord(ev_join, s)); SED_CHECK_HIP(hipStreamWaitEvent(st, ev_join, 0)); }
        return SED_OK;
    }
};

// ---- buffers of the recurrent tail: device pointers and sizes, filled by each orchestrator from its own layout ------------
struct RnnBufs {
    // saved context (forward writes, backward reads)
    const float* p2 = nullptr;                   // GRU input [B*T'][C], fp32 in every mode
    float *out[2] = {}, *gates[2] = {};          // per layer: [B*T'][2H]; r, z, n, gh_n
    float *logits_s = nullptr, *strong_sv = nullptr, *weak_sv = nullptr, *den_sv = nullptr;      // saved by the heads
    // H = 256 only
    float *gi[2] = {}, *wihT[2] = {};            // input projection [B*T'][2][3H]; the two W_ih stacked along K, transposed
    void *whh[2] = {}, *whhT[2] = {};            // grec.hip's bf16 layouts of W_hh
    void* xch[2] = {}; unsigned int* epoch[2] = {}; int* err = nullptr;      // ggru.hip: granules, epochs (ctx's / ws's: forward / backward), timeout flag
    // backward workspace (null in a forward)
    float *d_out = nullptr, *dgi[2] = {}, *dgh[2] = {}, *hprev[2] = {};
    float *d_in = nullptr, *dp2 = nullptr;       // dX of layer 1 / layer 0; H = 64: two direction planes each (gru4.hip)
    float *heads_part = nullptr, *gemm_part = nullptr;      // gemm_part: split-K partials of the weight-gradient batches, layer l
    size_t gemm_part_floats = 0, gemm_part_stride = 0; int splitk = 1;      // uses [l * stride, l * stride + floats); stride 0: shared
    double* zero = nullptr; int n_zero = 0;      // fp64 accumulators of the conv-block backward, cleared by the heads kernel
};

int rnn_forward(const Geo& g, const ParamOff& P, const float* params, const RnnBufs& R, int train, const uint64_t* seed_dev,
                float* strong, float* weak, int n_whh_packed, hipStream_t st);
// what rnn_forward / rnn_backward launch per layer for H = 64, and the heads' forward: one binding each, also re-launched alone
// by sed_kernel_replay (crnn.hip)
int rnn_gru_fwd64(const Geo& g, const ParamOff& P, const float* params, const RnnBufs& R, int l, int train, hipStream_t st);
int rnn_gru_bwd64(const Geo& g, const ParamOff& P, const float* params, const RnnBufs& R, int l, hipStream_t st);      // (not the fused-heads form)
int rnn_heads_fwd(const Geo& g, const ParamOff& P, const float* params, const RnnBufs& R, float* strong, float* weak, bool save,
                  int use_drop, const uint64_t* seed_dev, hipStream_t st);

// One backward call's view of the tail.  rnn_backward_plan fills it in (the fuse / defer_colsum / early_gru_w decisions are
// taken there and nowhere else); the orchestrator then calls rnn_backward in front of its conv-block half,
// rnn_deferred_weight_grads behind its block-2 wgrad launch and (crnn.hip) rnn_tail_weight_grads behind its block-1 wgrad launch.
struct RnnBwd {
    Geo g; ParamOff P; RnnBufs R;
    const float* params; float* grads; const uint64_t* seed_dev; const HeadsLoss* hl; const HeadsOut* ho; int parts; SideFork* side;
    bool fuse, defer_colsum, early_gru_w;
    const float* d_att;                          // dLoss/d(sof) [B][T'][NC] (sed_crnn_backward_att) or null: the heads kernel adds it
};
RnnBwd rnn_backward_plan(const Geo& g, const ParamOff& P, const RnnBufs& R, const float* params, float* grads,
                         const uint64_t* seed_dev, const HeadsLoss* hl, const HeadsOut* ho, int parts, SideFork* side,
                         const float* d_att = nullptr);
int rnn_backward(const RnnBwd& rb, const float* d_strong, const float* d_weak, hipStream_t st);
int rnn_weight_grads_layer(const RnnBwd& rb, int l, hipStream_t s2);      // GRU dW / db of one layer | of every layer, top down
int rnn_weight_grads(const RnnBwd& rb, hipStream_t s2);
int rnn_heads_colsum(const RnnBwd& rb, hipStream_t s2);                    // k_heads_colsum, or (fuse) k_heads_fin
int rnn_deferred_weight_grads(const RnnBwd& rb);                           // parts == 3: what rnn_backward left to the helper stream
int rnn_tail_weight_grads(const RnnBwd& rb);                               // ... and what goes behind the block-1 wgrad (k_gru_wgrad)

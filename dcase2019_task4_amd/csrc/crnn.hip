// crnn.hip - CRNN forward / backward orchestration behind the C-ABI (include/dcase_sed.h).
//
// Mirrors the operator sequence of CRNN.forward (baseline/models/CRNN.py:59-84):
//   conv block 0 (blk0.hip, fully fused) -> [conv3x3 + BN stats (conv.hip) -> BN/GLU/dropout/pool
//   (bnglu.hip)] x 2 -> BiGRU + heads (rnn.hip, shared with gcrnn.hip)
// All launches go to the caller's stream; no allocation, no synchronisation.
#include <stdarg.h>
#include <map>
#include <mutex>
#include <utility>
#include <stdio.h>
#include <string.h>
#include "common.h"
#include "kernels.h"
#include "gkernels.h"
#include "rnn.h"

static thread_local char g_err[512] = "";
void sed_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* sed_last_error(void) { return g_err; }
extern "C" int sed_version(void) { return 100; }
int g_sed_debug = 0;
extern "C" int sed_debug_set(int flags) { const int old = g_sed_debug; g_sed_debug = flags; return old; }

int sed_validate_dims(const sed_dims* d) {
    SED_CHECK_ARG(d != nullptr, "null dims");
    if (d->F != 64 || (d->C != 64 && d->C != 128) || (d->H != 64 && d->H != 256) ||
        (d->dtype != SED_DTYPE_F32 && d->dtype != SED_DTYPE_BF16 && d->dtype != SED_DTYPE_BF16X3 && d->dtype != SED_DTYPE_F16)) {
        sed_set_error("supported: F = 64, C in {64, 128}, H in {64, 256}, dtype in {f32, bf16, bf16x3, f16} (got F=%d C=%d H=%d dtype=%d)",
                      d->F, d->C, d->H, d->dtype);
        return SED_ERR_UNSUPPORTED;
    }
    SED_CHECK_ARG(d->B >= 1 && d->T >= 16, "need B >= 1 and T >= 16");
    SED_CHECK_ARG(d->nclass >= 1 && d->nclass <= 16, "nclass must be in [1, 16]");
    SED_CHECK_ARG(d->n_layers_rnn == 1 || d->n_layers_rnn == 2, "n_layers_rnn must be 1 or 2");
    SED_CHECK_ARG(d->p_drop >= 0.f && d->p_drop < 1.f, "p_drop must be in [0, 1)");
    SED_CHECK_ARG((int64_t)d->B * d->T * d->F * d->C < (1ll << 31), "batch too large for 32-bit pixel indices");
    return SED_OK;
}

ParamOff make_param_off(const Geo& g, int64_t* out) {
    ParamOff P;
    int64_t o = 0;
    int k = 0;
    auto put = [&](int64_t& field, int64_t n) {
        field = o;
        if (out) out[k] = o;
        ++k;
        o += n;
    };
    for (int i = 0; i < 3; ++i) {
        const int cin = (i == 0) ? 1 : g.C;
        put(P.conv_w[i], (int64_t)g.C * cin * 9);
        put(P.conv_b[i], g.C);
        put(P.bn_g[i], g.C);
        put(P.bn_b[i], g.C);
        put(P.glu_w[i], (int64_t)g.C * g.C);
        put(P.glu_b[i], g.C);
    }
    for (int l = 0; l < g.L; ++l) {
        const int nin = (l == 0) ? g.C : 2 * g.H;
        for (int dir = 0; dir < 2; ++dir) {
            put(P.w_ih[l][dir], (int64_t)3 * g.H * nin);
            put(P.w_hh[l][dir], (int64_t)3 * g.H * g.H);
            put(P.b_ih[l][dir], 3 * g.H);
            put(P.b_hh[l][dir], 3 * g.H);
        }
    }
    put(P.dense_w, (int64_t)g.NC * 2 * g.H);
    put(P.dense_b, g.NC);
    put(P.soft_w, (int64_t)g.NC * 2 * g.H);
    put(P.soft_b, g.NC);
    P.total = o;
    P.count = k;
    if (out) out[k] = o;
    return P;
}

CtxLayout make_ctx_layout(const Geo& g) {
    CtxLayout L;
    RegionCursor put;
    const size_t px[4] = {0, (size_t)g.B * g.H1 * g.W1, (size_t)g.B * g.H2 * g.W2, (size_t)g.B * g.T3};      // pixels of block i's OUTPUT: px[i + 1]
    put(L.acc0, 320 * sizeof(double));
    L.mom0 = L.acc0.sub(0, 64 * sizeof(double));
    L.stat[1] = L.acc0.sub(64 * sizeof(double), 128 * sizeof(double)); L.stat[2] = L.acc0.sub(192 * sizeof(double), 128 * sizeof(double));
    put(L.wz0, 64 * 12 * 4); put(L.wl0, 64 * 12 * 4); put(L.bn[0], 256 * 4);
    put(L.mompart, (size_t)x_moments_parts(g) * 54 * sizeof(double));
    put(L.p[0], px[1] * 64 * 4);
    for (int i = 1; i <= 2; ++i) {
        put(L.wpk[i], (9 + 16) * 4096 * 4); put(L.wpkT[i], (9 + 16) * 4096 * 4); put(L.y[i], px[i] * 64 * 4); put(L.bn[i], 256 * 4);
        put(L.p[i], px[i + 1] * 64 * 4);
    }
    const size_t bt = (size_t)g.B * g.T3;
    for (int l = 0; l < 2; ++l) {
        put(L.gates[l], bt * 512 * 4); put(L.out[l], bt * 128 * 4);      // (gi only exists in LDS, gru4.hip)
    }
    put(L.logits_s, bt * g.NC * 4); put(L.strong_sv, bt * g.NC * 4);
    put(L.weak_sv, (size_t)g.B * g.NC * 4); put(L.den_sv, (size_t)g.B * g.NC * 4);
    for (int i = 0; i < 3; ++i) put(L.mask[i], ((px[i + 1] + 3) / 4) * 2 * 64 * sizeof(uint16_t));
    L.total = put.o;
    return L;
}

WsLayout make_ws_layout(const Geo& g) {
    WsLayout W;
    RegionCursor put;
    const size_t n0 = (size_t)g.B * g.H1 * g.W1 * 64, n1 = (size_t)g.B * g.H2 * g.W2 * 64, bt = (size_t)g.B * g.T3;
    put(W.d_out, bt * 128 * 4);
    for (int l = 0; l < 2; ++l) { put(W.dgi[l], bt * 384 * 4); put(W.dgh[l], bt * 384 * 4); put(W.hprev[l], bt * 128 * 4); }
    put(W.d_in, 2 * bt * 128 * 4); put(W.heads_part, (size_t)g.B * 2 * (g.NC * 128 + g.NC) * 4);
    put(W.dp[2], 2 * bt * 64 * 4); put(W.dz[2], n1 * 4); put(W.dp[1], n1 * 4); put(W.dz[1], n0 * 4); put(W.dp[0], n0 * 4);
    put(W.pad0, 256 * sizeof(double)); put(W.coef[1], 192 * 4); put(W.coef[2], 192 * 4);
    const size_t glu = SED_GLUACC_N * sizeof(double);
    put(W.bwd_acc, 2 * glu + 2 * 64 * 10 * sizeof(double));      // every fp64 accumulator of the conv-block backward
    W.gluacc[1] = W.bwd_acc.sub(0, glu); W.gluacc[2] = W.bwd_acc.sub(glu, glu); W.de0 = W.bwd_acc.sub(2 * glu, 2 * 64 * 10 * sizeof(double));
    W.wgrad_blocks = SED_WGRAD_MAX_BLOCKS;
    put(W.wg_part, (size_t)W.wgrad_blocks * 9 * 4096 * 4);
    put(W.gemm_part, gemm_part_floats(4, SED_GRU_SPLITK, 192, 129) * 4);
    W.total = put.o;
    return W;
}

extern "C" int sed_param_count(const sed_dims* d) {
    if (sed_validate_dims(d) != SED_OK) return -1;
    const Geo g = make_geo(d);
    return make_param_off(g, nullptr).count;
}
extern "C" int sed_param_layout(const sed_dims* d, int64_t* offsets) {
    SED_TRY(sed_validate_dims(d));
    SED_CHECK_ARG(offsets != nullptr, "null offsets");
    const Geo g = make_geo(d);
    make_param_off(g, offsets);
    return SED_OK;
}
extern "C" size_t sed_crnn_ctx_bytes(const sed_dims* d) {
    if (sed_validate_dims(d) != SED_OK) return 0;
    const Geo g = make_geo(d);
    return g.generic ? gen_ctx_bytes(g) : make_ctx_layout(g).total;
}
extern "C" size_t sed_crnn_bwd_ws_bytes(const sed_dims* d) {
    if (sed_validate_dims(d) != SED_OK) return 0;
    const Geo g = make_geo(d);
    return g.generic ? gen_ws_bytes(g) : make_ws_layout(g).total;
}

extern "C" int sed_crnn_buffers_init(const sed_dims* d, void* ctx, size_t ctx_bytes, void* ws, size_t ws_bytes, void* stream) {
    SED_TRY(sed_validate_dims(d));
    const Geo g = make_geo(d);
    if (g.generic) return gen_buffers_init(g, ctx, ctx_bytes, ws, ws_bytes, (hipStream_t)stream);
    return SED_OK;                             // the specialised kernel set writes everything before it reads it
}

extern "C" int sed_crnn_ctx_view(const sed_dims* d, const char* name, size_t* offset, size_t* bytes) {
    SED_TRY(sed_validate_dims(d));
    SED_CHECK_ARG(name && offset && bytes, "null argument");
    const Geo g = make_geo(d);
    if (g.generic) return gen_ctx_view(g, name, offset, bytes);
    const CtxLayout L = make_ctx_layout(g);
    struct { const char* n; Region r; } tab[] = {
        {"mom0", L.mom0}, {"wz0", L.wz0}, {"wl0", L.wl0}, {"bn0", L.bn[0]},
        {"p0", L.p[0]}, {"y1", L.y[1]}, {"stat1", L.stat[1]}, {"bn1", L.bn[1]}, {"p1", L.p[1]},
        {"y2", L.y[2]}, {"stat2", L.stat[2]}, {"bn2", L.bn[2]}, {"p2", L.p[2]},
        {"gates0", L.gates[0]}, {"gates1", L.gates[1]}, {"gru0", L.out[0]}, {"gru1", L.out[1]},
        {"logits_s", L.logits_s}, {"den", L.den_sv},
    };
    for (auto& t : tab)
        if (strcmp(t.n, name) == 0) { *offset = t.r.off; *bytes = t.r.bytes; return SED_OK; }
    sed_set_error("sed_crnn_ctx_view: unknown buffer '%s'", name);
    return SED_ERR_BAD_ARG;
}

// The attention the heads of the forward that filled ctx pooled with (heads.hip: k_heads_attention): both kernel sets keep the
// attention logits of every frame in their ctx's "logits_s" region, whatever `train` and the MFMA dtype were.
extern "C" int sed_crnn_attention(const sed_dims* d, const void* ctx, size_t ctx_bytes, float* att, void* stream) {
    if (sed_validate_dims(d) != SED_OK) return SED_ERR_BAD_ARG;      // (the message says what is supported)
    SED_CHECK_ARG(ctx && att, "sed_crnn_attention: null argument");
    const size_t need = sed_crnn_ctx_bytes(d);
    if (ctx_bytes < need) {
        sed_set_error("sed_crnn_attention: ctx has %zu bytes, needs %zu", ctx_bytes, need);
        return SED_ERR_BAD_ARG;
    }
    size_t off = 0, bytes = 0;
    SED_TRY(sed_crnn_ctx_view(d, "logits_s", &off, &bytes));
    const Geo g = make_geo(d);
    return launch_heads_attention((const float*)((const char*)ctx + off), att, g.B * g.T3, g.NC, (hipStream_t)stream);
}

// ---- side stream: weight-gradient work that is off the backward critical path (rnn.h: SideFork) ----
// One helper stream + fork/join event pair exists per (device, caller stream): two host threads (or two models on two
// GPUs of one process) that call in on different streams never share events.  The pool is created under a mutex, on
// first use or - preferably, so that nothing is created while the caller's stream is being captured -
// by sed_stream_prepare(stream).
struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;          // backward
    // A second stream + event, created and never used.  They served a removed A/B schedule (a helper stream of their own
    // for the GRU weight gradients), but the streams a process creates decide which hardware queue the HIP runtime gives
    // each later stream, and without these two the waveform front-end's captured step crashed inside hipGraphLaunch when
    // two data-parallel ranks shared one GPU (tests/test_gpu_dp.py::test_waveform_front_end_world2).  Kept, in the same
    // creation order, until that runtime behaviour is understood.
    hipStream_t idle = nullptr;
    hipEvent_t idle_ev = nullptr;
    bool ok = false;
};
static std::mutex g_side_mu;
static std::map<std::pair<int, hipStream_t>, SideStream*> g_side;
struct ForkHook { void (*fn)(void*) = nullptr; void* user = nullptr; };        // sed_crnn_fork_callback, below
static std::map<std::pair<int, hipStream_t>, ForkHook> g_fork_hooks;
static SideStream& side_stream(hipStream_t caller) {
    static SideStream none;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return none;
    std::lock_guard<std::mutex> lk(g_side_mu);
    SideStream*& slot = g_side[std::make_pair(dev, caller)];
    if (slot == nullptr) {
        slot = new SideStream();
        // (default priority on purpose: a lowest-priority side stream, meant to let the critical-path kernels win the
        // CUs, made the replayed step 70 % slower - 1.79 vs 1.06 ms)
        if (hipStreamCreateWithFlags(&slot->s, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&slot->fork, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&slot->join, hipEventDisableTiming) == hipSuccess &&
            hipStreamCreateWithFlags(&slot->idle, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&slot->idle_ev, hipEventDisableTiming) == hipSuccess)
            slot->ok = true;
    }
    return *slot;
}
extern "C" int sed_stream_prepare(void* stream) {
    SideStream& sd = side_stream((hipStream_t)stream);
    if (!sd.ok) {
        sed_set_error("sed_stream_prepare: could not create the helper stream / events");
        return SED_ERR_LAUNCH;
    }
    return SED_OK;
}
// Releases what sed_stream_prepare / first use created for `stream` on the current device: the helper streams, their
// events and a pending fork hook.  The caller guarantees that no work of the library is in flight or being captured on the
// stream (synchronise it first); the stream can be prepared again afterwards.  A caller stream that was never prepared is a
// no-op.  hipStreamDestroy on a helper stream that still has work queued would complete it asynchronously, which is why the
// helper is synchronised here first - this is the ONE entry point of the library that blocks the host.
extern "C" int sed_stream_release(void* stream) {
    int dev = 0;
    SED_CHECK_HIP(hipGetDevice(&dev));
    SideStream* sd = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        const auto key = std::make_pair(dev, (hipStream_t)stream);
        auto it = g_side.find(key);
        if (it != g_side.end()) { sd = it->second; g_side.erase(it); }
        g_fork_hooks.erase(key);
    }
    if (sd == nullptr) return SED_OK;
    int rc = SED_OK;
    auto note = [&](hipError_t e) { if (e != hipSuccess && rc == SED_OK) { sed_set_error("sed_stream_release: %s", hipGetErrorString(e)); rc = SED_ERR_LAUNCH; } };
    if (sd->s) { note(hipStreamSynchronize(sd->s)); note(hipStreamDestroy(sd->s)); }
    if (sd->idle) note(hipStreamDestroy(sd->idle));
    if (sd->fork) note(hipEventDestroy(sd->fork));
    if (sd->join) note(hipEventDestroy(sd->join));
    if (sd->idle_ev) note(hipEventDestroy(sd->idle_ev));
    delete sd;
    return rc;
}
// One-shot hook for a caller with independent work to run BESIDE the recurrent part of a forward (the waveform front-end:
// the next batch's STFT, features.WaveformFrontEnd): the next sed_crnn_forward on `stream` calls fn(user) on the calling host
// thread after enqueueing its last conv-block kernel and before enqueueing its first recurrence kernel.  The callback forks
// its own stream off `stream` there (event record + wait) and enqueues its work, so the fork sits at that point of the
// enqueue ORDER too: a hipGraph captured around the forward submits its nodes in creation order, and a dependency on a node in
// the middle of another stream's chain that is submitted late starts late (measured: a fork expressed only as an event
// recorded here and waited for after the forward returned started 300 us late, at the first backward kernel).
extern "C" int sed_crnn_fork_callback(void* stream, void (*fn)(void*), void* user) {
    int dev = 0;
    SED_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_side_mu);
    const auto key = std::make_pair(dev, (hipStream_t)stream);
    if (fn == nullptr) { g_fork_hooks.erase(key); return SED_OK; }
    ForkHook& h = g_fork_hooks[key];
    h.fn = fn;
    h.user = user;
    return SED_OK;
}
int sed_fork_point(hipStream_t st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return SED_OK;
    ForkHook h;
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        auto it = g_fork_hooks.find(std::make_pair(dev, st));
        if (it == g_fork_hooks.end()) return SED_OK;
        h = it->second;
        g_fork_hooks.erase(it);
    }
    if (h.fn) h.fn(h.user);
    return SED_OK;
}
// one backward call's handle (SED_DEBUG_NO_SIDE_STREAM: every kernel on the caller's stream, for near-solo kernel times)
static SideFork side_fork(hipStream_t st) {
    SideStream& sd = side_stream(st);
    const bool ok = sd.ok && !(g_sed_debug & SED_DEBUG_NO_SIDE_STREAM);
    return SideFork{ok ? sd.s : st, sd.fork, sd.join, ok, false};
}

// ---- one call of the specialised fp32 kernel set -------------------------------------------------------------------------
// Each stage_* function below holds the ONE launch_* call of its stage, bound to the buffers of a Call.  sed_crnn_forward,
// crnn_backward_impl and sed_kernel_replay are sequences of stage calls: what differs between them is an argument of the stage.
struct Call {
    Geo g; ParamOff P; CtxLayout L; WsLayout W;
    const float* params; float* grads; const float* x; const uint64_t* seed_dev; void* ctx; void* ws;      // grads, ws: null in a forward
    int H(int i) const { return i == 1 ? g.H1 : g.H2; }       // the image of conv block i = 1, 2
    int Wd(int i) const { return i == 1 ? g.W1 : g.W2; }
    int fwd_drop(int train) const { return (train && g.p > 0.f) ? 1 : 0; }
    int bwd_drop() const { return (g.p > 0.f) ? 1 : 0; }
};

// the recurrent tail's buffers in the specialised layouts
static RnnBufs rnn_bufs(const Call& c) {
    const CtxLayout& L = c.L; const WsLayout& W = c.W; void* ctx = c.ctx; void* ws = c.ws;
    RnnBufs R;
    R.p2 = L.p[2].f(ctx);
    for (int l = 0; l < 2; ++l) { R.out[l] = L.out[l].f(ctx); R.gates[l] = L.gates[l].f(ctx); }
    R.logits_s = L.logits_s.f(ctx); R.strong_sv = L.strong_sv.f(ctx); R.weak_sv = L.weak_sv.f(ctx); R.den_sv = L.den_sv.f(ctx);
    if (ws == nullptr) return R;
    R.d_out = W.d_out.f(ws); R.d_in = W.d_in.f(ws); R.dp2 = W.dp[2].f(ws); R.heads_part = W.heads_part.f(ws);
    for (int l = 0; l < 2; ++l) { R.dgi[l] = W.dgi[l].f(ws); R.dgh[l] = W.dgh[l].f(ws); R.hprev[l] = W.hprev[l].f(ws); }
    R.gemm_part = W.gemm_part.f(ws); R.gemm_part_floats = W.gemm_part.bytes / 4; R.splitk = SED_GRU_SPLITK;
    R.zero = W.bwd_acc.d(ws); R.n_zero = (int)(W.bwd_acc.bytes / sizeof(double));
    return R;
}

// running: the block's running [mean | var] (the replay hands 128 floats that an update = 0 launch never touches)
static int stage_blk0_fwd(const Call& c, float* running, int64_t* tracked, int train, int upd, const ConvPackArgs* pack,
                          int main_kernel_only, int mom_ready, hipStream_t st) {
    const ParamOff& P = c.P; const CtxLayout& L = c.L; void* ctx = c.ctx;
    return launch_blk0_forward(c.g, c.x, c.params + P.conv_w[0], c.params + P.conv_b[0], c.params + P.bn_g[0], c.params + P.bn_b[0],
                               c.params + P.glu_w[0], c.params + P.glu_b[0], running, running + 64, tracked, train, upd, c.seed_dev,
                               L.mom0.d(ctx), L.mompart.d(ctx), L.wz0.f(ctx), L.wl0.f(ctx), L.bn[0].f(ctx), L.p[0].f(ctx),
                               c.fwd_drop(train) ? L.mask[0].m(ctx) : nullptr, pack, st, main_kernel_only, nullptr, nullptr, mom_ready);
}
static int stage_conv_fwd(const Call& c, int i, bool with_stat, int zero_stat, hipStream_t st) {
    const CtxLayout& L = c.L; void* ctx = c.ctx;
    return launch_conv_fwd(L.p[i - 1].f(ctx), L.wpk[i].f(ctx), c.params + c.P.conv_b[i], L.y[i].f(ctx), with_stat ? L.stat[i].d(ctx) : nullptr,
                           zero_stat, c.g.B, c.H(i), c.Wd(i), st);
}
static int stage_glu_fwd(const Call& c, int i, float* running, int64_t* tracked, int train, int upd, hipStream_t st) {
    const Geo& g = c.g; const ParamOff& P = c.P; const CtxLayout& L = c.L; void* ctx = c.ctx;
    const int use_drop = c.fwd_drop(train);
    return launch_glu_pool_fwd(L.y[i].f(ctx), L.stat[i].d(ctx), (double)g.B * c.H(i) * c.Wd(i), c.params + P.bn_g[i], c.params + P.bn_b[i],
                               running, running + 64, tracked, train, upd, g.eps, g.mom, L.bn[i].f(ctx), c.params + P.glu_w[i],
                               c.params + P.glu_b[i], L.p[i].f(ctx), g.B, c.H(i), c.Wd(i), i, use_drop, g.p, c.seed_dev,
                               use_drop ? L.mask[i].m(ctx) : nullptr, st);
}
// prep_out != null: the BatchNorm-backward coefficients and the block's parameter gradients are left to the conv dgrad / wgrad
// kernels (BnBwdPrepArgs, kernels.h); null: k_bn_bwd_prep follows
static int stage_glu_bwd(const Call& c, int i, int zero_acc, BnBwdPrepArgs* prep_out, hipStream_t st) {
    const Geo& g = c.g; const ParamOff& P = c.P; const CtxLayout& L = c.L; const WsLayout& W = c.W; void* ctx = c.ctx; void* ws = c.ws;
    // (block 2: the GRU's dX arrives as two direction planes)
    return launch_glu_pool_bwd(L.y[i].f(ctx), L.bn[i].f(ctx), c.params + P.glu_w[i], c.params + P.glu_b[i], W.dp[i].f(ws),
                               i == 2 ? W.dp[i].f(ws) + (size_t)g.B * g.T3 * 64 : nullptr, W.dz[i].f(ws), W.gluacc[i].d(ws), zero_acc, g.B,
                               c.H(i), c.Wd(i), c.bwd_drop(), g.p, L.mask[i].m(ctx), c.params + P.bn_g[i], W.coef[i].f(ws),
                               c.grads + P.bn_g[i], c.grads + P.bn_b[i], c.grads + P.glu_w[i], c.grads + P.glu_b[i], c.grads + P.conv_b[i],
                               prep_out, st);
}
static int stage_conv_dgrad(const Call& c, int i, const BnBwdPrepArgs* prep, hipStream_t st) {
    const WsLayout& W = c.W;
    return launch_conv_dgrad(W.dz[i].f(c.ws), c.L.y[i].f(c.ctx), W.coef[i].f(c.ws), c.L.wpkT[i].f(c.ctx), W.dp[i - 1].f(c.ws), c.g.B, c.H(i),
                             c.Wd(i), prep, st);
}
static int stage_conv_wgrad(const Call& c, int i, const BnBwdPrepArgs* prep, hipStream_t st) {
    const WsLayout& W = c.W;
    return launch_conv_wgrad(W.dz[i].f(c.ws), c.L.y[i].f(c.ctx), W.coef[i].f(c.ws), c.L.p[i - 1].f(c.ctx), W.wg_part.f(c.ws), W.wgrad_blocks,
                             c.grads + c.P.conv_w[i], c.g.B, c.H(i), c.Wd(i), prep, st);
}
static int stage_blk0_bwd(const Call& c, int zero_de, hipStream_t st) {
    const ParamOff& P = c.P; const CtxLayout& L = c.L; void* ctx = c.ctx;
    return launch_blk0_backward(c.g, c.x, c.params + P.conv_w[0], c.params + P.conv_b[0], c.params + P.bn_g[0], c.params + P.bn_b[0],
                                c.params + P.glu_w[0], L.mask[0].m(ctx), L.mom0.d(ctx), L.wz0.f(ctx), L.wl0.f(ctx), L.bn[0].f(ctx),
                                c.W.dp[0].f(c.ws), c.W.de0.d(c.ws), zero_de, c.grads + P.conv_w[0], c.grads + P.conv_b[0],
                                c.grads + P.bn_g[0], c.grads + P.bn_b[0], c.grads + P.glu_w[0], c.grads + P.glu_b[0], st);
}

extern "C" int sed_crnn_forward(const sed_dims* d, const float* params, float* bn_running, int64_t* bn_tracked,
                                const float* x, int train, int update_bn, const uint64_t* seed_dev, void* ctx,
                                size_t ctx_bytes, float* strong, float* weak, void* stream) {
    SED_TRY(sed_validate_dims(d));
    SED_CHECK_ARG(params && bn_running && x && ctx, "sed_crnn_forward: null argument");
    // train bit 2 (value 4): this batch's patch moments are already in ctx (sed_crnn_moments ran for it, e.g. during the previous
    // step): no moments launch at the head of the forward
    const int mom_ready = (train & 4) ? 1 : 0;
    train &= 3;
    // strong == weak == NULL (train mode only): the output heads are left to sed_mt_step_backward, which runs them together
    // with the loss and their backward in front of the top layer's backward recurrence
    SED_CHECK_ARG((strong && weak) || (!strong && !weak && train), "sed_crnn_forward: strong and weak must both be given (or both NULL in train mode: heads deferred)");
    const Geo g = make_geo(d);
    const ParamOff P = make_param_off(g, nullptr);
    if (g.generic) {
        SED_CHECK_ARG(!(train && g.p > 0.f) || seed_dev, "sed_crnn_forward: dropout enabled but seed_dev is null");
        side_stream((hipStream_t)stream);      // (first use creates the helper streams here, as ever: their ORDER matters, see SideStream)
        return gen_forward(g, P, params, bn_running, bn_tracked, x, train | (mom_ready ? 4 : 0), update_bn, seed_dev, ctx, ctx_bytes, strong,
                           weak, (hipStream_t)stream);
    }
    const Call c = {g, P, make_ctx_layout(g), make_ws_layout(g), params, nullptr, x, seed_dev, ctx, nullptr};
    const CtxLayout& L = c.L;
    if (ctx_bytes < L.total) {
        sed_set_error("sed_crnn_forward: ctx has %zu bytes, needs %zu", ctx_bytes, L.total);
        return SED_ERR_WORKSPACE;
    }
    SED_CHECK_ARG(!c.fwd_drop(train) || seed_dev, "sed_crnn_forward: dropout enabled but seed_dev is null");
    hipStream_t st = (hipStream_t)stream;
    const int upd = (train && update_bn) ? 1 : 0;
    auto trk = [&](int i) { return bn_tracked ? bn_tracked + i : nullptr; };

    // conv1 / conv2 weights -> [tap][ci][co] + Winograd panels (+ flipped/transposed copies for dgrad); the same threads
    // also zero the fp64 BatchNorm sums of blocks 1 and 2.  In a training forward this rides along in the k_x_moments
    // launch (independent work, extra workgroups) instead of being a launch of its own on the chain.
    const ConvPackArgs pack = {params + P.conv_w[1], params + P.conv_w[2], L.wpk[1].f(ctx), L.wpk[2].f(ctx),
                               train ? L.wpkT[1].f(ctx) : nullptr, train ? L.wpkT[2].f(ctx) : nullptr, L.stat[1].d(ctx), train ? 256 : 0};
    // ---- conv block 0 ---------------------------------------------------------------------------
    SED_TRY(stage_blk0_fwd(c, bn_running, trk(0), train, upd, train ? &pack : nullptr, 0, mom_ready, st));
    if (!train) SED_TRY(launch_conv_pack(pack, st));      // (training: done by extra workgroups of k_x_moments / k_blk0_prep_pack)
    // ---- conv blocks 1, 2 -----------------------------------------------------------------------
    for (int i = 1; i <= 2; ++i) {
        SED_TRY(stage_conv_fwd(c, i, train != 0, 0, st));
        SED_TRY(stage_glu_fwd(c, i, bn_running + 2 * i * 64, trk(i), train, upd, st));
    }
    // ---- BiGRU + heads --------------------------------------------------------------------------
    return rnn_forward(g, P, params, rnn_bufs(c), train, seed_dev, strong, weak, 0, st);
}

// The train-mode BatchNorm statistics of conv block 0 come from the 9 + 45 first / second moments of the 3x3 input patch
// (blk0.hip): a function of the BATCH only, not of any parameter.  A caller that has the next batch resident while the current
// step runs (features.WaveformFrontEnd: one batch ahead; a constant / resident batch) computes them THEN - beside the
// recurrences, which leave most of the chip idle - and passes train | 4 to the forward that consumes them: 16 us (B = 24) of
// launch + round trip leave the head of the step's critical chain.  Same kernel, same partials, same order: bit-identical.
extern "C" int sed_crnn_moments(const sed_dims* d, const float* x, void* ctx, size_t ctx_bytes, void* stream) {
    SED_TRY(sed_validate_dims(d));
    SED_CHECK_ARG(x && ctx, "sed_crnn_moments: null argument");
    const Geo g = make_geo(d);
    double* mompart = nullptr;
    if (g.generic) {
        SED_TRY(gen_mompart(g, ctx, ctx_bytes, &mompart));
    } else {
        const CtxLayout L = make_ctx_layout(g);
        if (ctx_bytes < L.total) {
            sed_set_error("sed_crnn_moments: ctx has %zu bytes, needs %zu", ctx_bytes, L.total);
            return SED_ERR_WORKSPACE;
        }
        mompart = L.mompart.d(ctx);
    }
    return launch_x_moments(g, x, mompart, nullptr, (hipStream_t)stream);
}

static int crnn_backward_impl(const sed_dims* d, const float* params, const float* x, const uint64_t* seed_dev,
                              void* ctx, size_t ctx_bytes, const float* d_strong, const float* d_weak, float* grads,
                              void* ws, size_t ws_bytes, int parts, void* stream, const HeadsLoss* hl,
                              const HeadsOut* ho = nullptr, const float* d_att = nullptr) {
    SED_TRY(sed_validate_dims(d));
    SED_CHECK_ARG(params && x && ctx && (hl || (d_strong && d_weak)) && grads && ws, "sed_crnn_backward: null argument");
    SED_CHECK_ARG(parts == 1 || parts == 2 || parts == 3 || parts == 5 || parts == 8,
                  "sed_crnn_backward: parts must be 1, 2, 3, 5 or 8");
    const Geo g = make_geo(d);
    const ParamOff P = make_param_off(g, nullptr);
    if (g.generic) {
        SED_CHECK_ARG(!(g.p > 0.f) || seed_dev, "sed_crnn_backward: dropout enabled but seed_dev is null");
        SideFork side0 = side_fork((hipStream_t)stream);
        return gen_backward(g, P, params, x, seed_dev, ctx, ctx_bytes, d_strong, d_weak, grads, ws, ws_bytes, parts, (hipStream_t)stream,
                            side0, hl, ho, d_att);
    }
    const Call c = {g, P, make_ctx_layout(g), make_ws_layout(g), params, grads, x, seed_dev, ctx, ws};
    const WsLayout& W = c.W;
    if (ctx_bytes < c.L.total || ws_bytes < W.total) {
        sed_set_error("sed_crnn_backward: ctx %zu/%zu bytes, ws %zu/%zu bytes", ctx_bytes, c.L.total, ws_bytes, W.total);
        return SED_ERR_WORKSPACE;
    }
    SED_CHECK_ARG(!c.bwd_drop() || seed_dev, "sed_crnn_backward: dropout enabled but seed_dev is null");
    hipStream_t st = (hipStream_t)stream;
    SideFork side = side_fork(st);
    // ---- heads, BiGRU (+ the weight-gradient tail of a parts == 1 / parts == 8 call) --------------
    const RnnBwd rb = rnn_backward_plan(g, P, rnn_bufs(c), params, grads, seed_dev, hl, ho, parts, &side, d_att);
    SED_TRY(rnn_backward(rb, d_strong, d_weak, st));
    if (!(parts & 2)) return SED_OK;
    // ---- conv blocks 2, 1 -----------------------------------------------------------------------
    // every fp64 accumulator of the conv-block backward: zeroed by k_heads_bwd when this call also ran part 1
    if (!(parts & 1)) SED_CHECK_HIP(hipMemsetAsync(W.bwd_acc.d(ws), 0, W.bwd_acc.bytes, st));
    // Stream schedule (kernel timeline of one step, tools/timeline.py): the dgrad chain is the critical path.
    //   main: glu2_bwd  prep | dgrad2            | glu1_bwd  prep | dgrad1          | blk0_bwd  finalize |
    //   side:                | wgrad2  heads_fin |                | wgrad1  reduce  GRU dW/db  reduce    | join
    // (Forking before glu2_bwd so that the GRU GEMMs run first and wgrad1 starts on time measured slower, 1.061 vs
    // 1.029 ms: they then compete with the critical-path kernels glu2_bwd / dgrad2 / glu1_bwd.)
    // (Same experiment again with the Winograd convolutions, where the side stream has become the tail of the step: still
    // slower, 28.0 vs 28.3 k clips/s.)
    // (Starting wgrad1 only after dgrad1, next to the VALU-bound k_blk0_bwd, measured the same: dgrad1 drops from
    // 175 to 93 us but k_blk0_bwd, left with one wave per SIMD beside the wgrad wave, goes from 86 to 177 us.)
    // BatchNorm-backward coefficients: derived by the conv dgrad / wgrad kernels themselves from the reduction sums (no
    // 1-workgroup k_bn_bwd_prep + launch gap between the GLU backward and the dgrad, twice per step); the direct conv
    // kernels need the separate kernel
    const bool fuse_prep = (g_sed_debug & (SED_DEBUG_DIRECT_CONV | SED_DEBUG_DIRECT_WGRAD)) == 0;
    BnBwdPrepArgs prep[3] = {};
    for (int i = 2; i >= 1; --i) {
        BnBwdPrepArgs* pp = fuse_prep ? &prep[i] : nullptr;
        SED_TRY(stage_glu_bwd(c, i, 0, pp, st));
        // block 2: the dgrad - the critical chain - is captured between the two halves of the fork (SideFork); block 1: behind both
        SED_TRY(side.mark(st));
        if (i == 1) SED_TRY(side.start());
        SED_TRY(stage_conv_dgrad(c, i, pp, st));
        if (i == 2) SED_TRY(side.start());
        SED_TRY(stage_conv_wgrad(c, i, pp, side.s));
        if (i == 2) SED_TRY(rnn_deferred_weight_grads(rb));      // parts == 3: head column sum behind wgrad2
        if (i == 1) SED_TRY(rnn_tail_weight_grads(rb));          // parts == 3: every GRU dW / db at the very end of the helper stream
    }
    // ---- conv block 0 ---------------------------------------------------------------------------
    SED_TRY(stage_blk0_bwd(c, 0, st));
    return side.join(st);
}

extern "C" int sed_crnn_backward(const sed_dims* d, const float* params, const float* x, const uint64_t* seed_dev,
                                 void* ctx, size_t ctx_bytes, const float* d_strong, const float* d_weak, float* grads,
                                 void* ws, size_t ws_bytes, int parts, void* stream) {
    return crnn_backward_impl(d, params, x, seed_dev, ctx, ctx_bytes, d_strong, d_weak, grads, ws, ws_bytes, parts, stream, nullptr);
}

// sed_crnn_backward with one more upstream gradient, d_att = dLoss/d(sof) (what sed_crnn_attention returns), added in the heads
// backward (heads.hip: k_heads_bwd_att); d_att == NULL enqueues exactly what sed_crnn_backward does.  A parts value without the
// heads (2, 8) has no use for it.
extern "C" int sed_crnn_backward_att(const sed_dims* d, const float* params, const float* x, const uint64_t* seed_dev,
                                     void* ctx, size_t ctx_bytes, const float* d_strong, const float* d_weak, const float* d_att,
                                     float* grads, void* ws, size_t ws_bytes, int parts, void* stream) {
    return crnn_backward_impl(d, params, x, seed_dev, ctx, ctx_bytes, d_strong, d_weak, grads, ws, ws_bytes, parts, stream, nullptr,
                              nullptr, d_att);
}

// the argument checks and the loss inputs that sed_mt_loss_backward and sed_mt_step_backward share
static int heads_loss_args(HeadsLoss& hl, const sed_dims* d, const float* strong_ema, const float* weak_ema, const float* target, int weak_lo,
                           int weak_hi, int strong_lo, int strong_hi, sed_step_state* state_dev, int advance_state, float* losses,
                           float* d_strong, float* d_weak, int parts) {
    SED_CHECK_ARG(d && strong_ema && weak_ema && target && state_dev && losses, "fused loss + backward: null argument");
    SED_CHECK_ARG(parts == 1 || parts == 3 || parts == 5, "fused loss + backward: parts must include the heads (1, 3 or 5)");
    SED_CHECK_ARG(weak_lo >= 0 && weak_hi <= d->B && weak_lo <= weak_hi && strong_lo >= 0 && strong_hi <= d->B &&
                      strong_lo <= strong_hi, "fused loss + backward: bad mask range");
    hl = {strong_ema, weak_ema, target, weak_lo, weak_hi, strong_lo, strong_hi, state_dev, losses, d_strong, d_weak,
          advance_state ? state_dev : nullptr};
    return SED_OK;
}

extern "C" int sed_mt_loss_backward(const sed_dims* d, const float* params, const float* x, const uint64_t* seed_dev,
                                    void* ctx, size_t ctx_bytes, const float* strong_ema, const float* weak_ema,
                                    const float* target, int weak_lo, int weak_hi, int strong_lo, int strong_hi,
                                    sed_step_state* state_dev, int advance_state, float* losses, float* d_strong,
                                    float* d_weak, float* grads, void* ws, size_t ws_bytes, int parts, void* stream) {
    HeadsLoss hl;
    SED_TRY(heads_loss_args(hl, d, strong_ema, weak_ema, target, weak_lo, weak_hi, strong_lo, strong_hi, state_dev, advance_state, losses,
                            d_strong, d_weak, parts));
    return crnn_backward_impl(d, params, x, seed_dev, ctx, ctx_bytes, nullptr, nullptr, grads, ws, ws_bytes, parts, stream, &hl);
}

extern "C" int sed_mt_step_backward(const sed_dims* d, const float* params, const float* x, const uint64_t* seed_dev,
                                    void* ctx, size_t ctx_bytes, float* strong, float* weak, const float* strong_ema,
                                    const float* weak_ema, const float* target, int weak_lo, int weak_hi, int strong_lo,
                                    int strong_hi, sed_step_state* state_dev, int advance_state, float* losses, float* d_strong,
                                    float* d_weak, float* grads, void* ws, size_t ws_bytes, int parts, void* stream) {
    SED_CHECK_ARG(strong && weak, "sed_mt_step_backward: null argument");
    HeadsLoss hl;
    SED_TRY(heads_loss_args(hl, d, strong_ema, weak_ema, target, weak_lo, weak_hi, strong_lo, strong_hi, state_dev, advance_state, losses,
                            d_strong, d_weak, parts));
    HeadsOut ho = {strong, weak};
    return crnn_backward_impl(d, params, x, seed_dev, ctx, ctx_bytes, nullptr, nullptr, grads, ws, ws_bytes, parts, stream, &hl, &ho);
}

extern "C" int sed_kernel_replay(const char* name, const sed_dims* d, const float* params, const float* x,
                                 const uint64_t* seed_dev, void* ctx, size_t ctx_bytes, float* grads, void* ws,
                                 size_t ws_bytes, void* stream) {
    SED_TRY(sed_validate_dims(d));
    SED_CHECK_ARG(name && params && x && ctx && grads && ws, "sed_kernel_replay: null argument");
    const Geo g = make_geo(d);
    if (g.generic) {
        sed_set_error("sed_kernel_replay: only the C = 64 / H = 64 / fp32 kernel set is replayable");
        return SED_ERR_UNSUPPORTED;
    }
    const Call c = {g, make_param_off(g, nullptr), make_ctx_layout(g), make_ws_layout(g), params, grads, x, seed_dev, ctx, ws};
    if (ctx_bytes < c.L.total || ws_bytes < c.W.total) {
        sed_set_error("sed_kernel_replay: buffers too small");
        return SED_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    // a training launch that updates no running statistics: the running-stat pointers get 128 floats it never touches
    float* no_running = c.W.coef[1].f(ws);
    auto is = [&](const char* n) { return strcmp(name, n) == 0; };
    auto is_k = [&](const char* fmt, int k) {
        char nm[32];
        snprintf(nm, sizeof nm, fmt, k);
        return is(nm);
    };
    if (is("x_moments")) return sed_crnn_moments(d, x, ctx, ctx_bytes, stream);
    // (the folded weights of the last real forward are still in wz0 / wl0: the main kernel only)
    if (is("blk0_fwd")) return stage_blk0_fwd(c, no_running, nullptr, 1, 0, nullptr, 1, 0, st);
    for (int i = 1; i <= 2; ++i) {
        if (is_k("conv%d_fwd", i)) return stage_conv_fwd(c, i, true, 1, st);
        if (is_k("glu%d_fwd", i)) return stage_glu_fwd(c, i, no_running, nullptr, 1, 0, st);
        if (is_k("glu%d_bwd", i)) return stage_glu_bwd(c, i, 1, nullptr, st);
        if (is_k("conv%d_wgrad", i)) return stage_conv_wgrad(c, i, nullptr, st);
        if (is_k("conv%d_dgrad", i)) return stage_conv_dgrad(c, i, nullptr, st);
    }
    const RnnBufs R = rnn_bufs(c);
    for (int l = 0; l < g.L; ++l) {
        if (is_k("gru%d_fwd", l)) return rnn_gru_fwd64(g, c.P, params, R, l, 1, st);
        if (is_k("gru%d_bwd", l)) return rnn_gru_bwd64(g, c.P, params, R, l, st);
    }
    // (the posteriors go where a training forward saves them)
    if (is("heads_fwd")) return rnn_heads_fwd(g, c.P, params, R, R.strong_sv, R.weak_sv, false, c.bwd_drop(), seed_dev, st);
    if (is("gru_wgrad")) {
        // every GRU dW / db, as a parts == 1 backward issues them (rnn.hip: one k_gru_wgrad launch + its reduce)
        SideFork side = side_fork(st);
        return rnn_weight_grads(rnn_backward_plan(g, c.P, R, params, grads, seed_dev, nullptr, nullptr, 1, &side), st);
    }
    if (is("blk0_bwd")) return stage_blk0_bwd(c, 1, st);
    sed_set_error("sed_kernel_replay: unknown kernel '%s'", name);
    return SED_ERR_BAD_ARG;
}

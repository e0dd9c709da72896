// gcrnn.hip - CRNN forward / backward orchestration of the GENERIC kernel set (gen.h) behind the same C-ABI entry
// points as crnn.hip (which dispatches here for every configuration other than C = 64 / H = 64 / fp32).
//
// Operator sequence = CRNN.forward (baseline/models/CRNN.py:59-84) with nb_filters = [C, C, C], n_RNN_cell = H:
//   block 0 (blk0.hip, templated on C; always fp32) -> [conv3x3 + BN sums (gconv.hip) -> BN / GLU / dropout / pool
//   (gglu.hip)] x 2 -> BiGRU + heads (rnn.hip, shared with crnn.hip).
#include <string.h>
#include "common.h"
#include "kernels.h"
#include "gkernels.h"
#include "gpack.h"
#include "rnn.h"

// bytes per element of the packed weights (wpk, wpkT, wg, wgT) and of the conv-block activations / gradients in HBM (p0, y1,
// p1, y2; dz1, dz2, dp0, dp1): bf16 in SED_DTYPE_BF16 mode, fp32 otherwise (gen.h Stor<>); p2 - the GRU input - and dp2 are
// always fp32
static inline size_t esz(const Geo& g) { return g.mode == SED_DTYPE_BF16 ? 2 : 4; }
static inline int gru_splitk(const Geo& g) { return g.H == 64 ? SED_GRU_SPLITK : 4; }
// split-K partials of the GRU weight-gradient batch: the W_ih problems have N = nin (C, or 2H for layer 1), the W_hh
// problems N = H - the batch's stride is set by the LARGEST of them (with one layer and H > C that is H, not C)
static inline size_t gru_gemm_part_floats(const Geo& g) {
    int max_n = g.H > g.C ? g.H : g.C;
    if (g.L > 1 && 2 * g.H > max_n) max_n = 2 * g.H;
    return gemm_part_floats(4, gru_splitk(g), 3 * g.H, max_n + 1);
}

struct GCtx {
    Region acc0, mom0, stat[3];               // fp64: patch moments of block 0 | BatchNorm sums of blocks 1, 2
    Region wz0, wl0, mompart;
    Region wpk[3], wpkT[3], wg[3], wgT[3], bg[3], y[3];      // index 1, 2
    Region bn[3], p[3];                       // index 0, 1, 2
    Region ph[2], yh[3];                      // SED_DTYPE_F16: the forward chain's fp16 p0, p1 / y1, y2 (p[], y[] are then the bf16 copies the backward reads)
    Region gi[2], gates[2], out[2], whh[2], whhT[2];
    Region wihT[2];                           // [nin][6H]: the two W_ih stacked along K and transposed (dX GEMM operand)
    Region xch[2], epoch[2], err;             // cluster recurrence: exchange granules, launch epochs, spin-timeout flag
    Region logits_s, strong_sv, weak_sv, den_sv;
    Region mask[3];
    size_t total;
};
static size_t mask_bytes(size_t Q, int C) { return ((Q + 3) / 4) * (size_t)(C / 32) * 64 * sizeof(uint16_t); }

static GCtx make_gctx(const Geo& g) {
    GCtx L;
    RegionCursor put;
    const size_t C = g.C, H = g.H, E = esz(g);
    const size_t n0 = (size_t)g.B * g.H1 * g.W1 * C, n1 = (size_t)g.B * g.H2 * g.W2 * C, n2 = (size_t)g.B * g.T3 * C;
    put(L.acc0, (64 + 4 * C) * sizeof(double));
    L.mom0 = L.acc0.sub(0, 64 * sizeof(double));
    L.stat[1] = L.acc0.sub(64 * sizeof(double), 2 * C * sizeof(double)); L.stat[2] = L.acc0.sub((64 + 2 * C) * sizeof(double), 2 * C * sizeof(double));
    put(L.wz0, C * 12 * 4); put(L.wl0, C * 12 * 4); put(L.bn[0], 4 * C * 4);
    put(L.mompart, (size_t)x_moments_parts(g) * 54 * sizeof(double));
    put(L.p[0], n0 * E);
    const size_t nn[3] = {0, n0, n1}, np[3] = {n0, n1, n2};
    for (int i = 1; i <= 2; ++i) {
        put(L.wpk[i], 9 * C * C * E); put(L.wpkT[i], 9 * C * C * E); put(L.wg[i], C * C * E); put(L.wgT[i], C * C * E);
        put(L.bg[i], C * 4); put(L.y[i], nn[i] * E); put(L.bn[i], 4 * C * 4); put(L.p[i], np[i] * (i == 2 ? 4 : E));
    }
    if (g.f16) { put(L.ph[0], n0 * 2); put(L.yh[1], n0 * 2); put(L.ph[1], n1 * 2); put(L.yh[2], n1 * 2); }
    const size_t bt = (size_t)g.B * g.T3;
    for (int l = 0; l < 2; ++l) {
        put(L.gi[l], g.H == 64 ? 0 : bt * 6 * H * 4);          // (H = 64: the projection runs inside gru4.hip's kernel)
        put(L.gates[l], bt * 8 * H * 4); put(L.out[l], bt * 2 * H * 4);
        // (whh / whhT: sized for the fp32 packing of the streaming recurrence, removed; only grec.hip's bf16 layouts use them now)
        put(L.whh[l], g.H == 64 ? 0 : 2 * 3 * H * H * 4); put(L.whhT[l], g.H == 64 ? 0 : 2 * 3 * H * H * 4);
        put(L.xch[l], g.H == 256 ? gclu_xch_bytes(g.B, g.H, 0) : 0); put(L.epoch[l], (size_t)2 * g.B * 4);
        put(L.wihT[l], g.H == 64 ? 0 : (size_t)(l == 0 ? C : 2 * H) * 6 * H * 4);
    }
    put(L.err, 256);
    put(L.logits_s, bt * g.NC * 4); put(L.strong_sv, bt * g.NC * 4);
    put(L.weak_sv, (size_t)g.B * g.NC * 4); put(L.den_sv, (size_t)g.B * g.NC * 4);
    put(L.mask[0], mask_bytes((size_t)g.B * g.H1 * g.W1, g.C)); put(L.mask[1], mask_bytes((size_t)g.B * g.H2 * g.W2, g.C));
    put(L.mask[2], mask_bytes((size_t)g.B * g.T3, g.C));
    L.total = put.o;
    return L;
}

struct GWs {
    Region d_out, dgi[2], dgh[2], hprev[2], d_in, heads_part;
    Region dp[3], dz[3], coef[3];             // dp[i]: gradient w.r.t. block i's pooled output; dz / coef: blocks 1, 2
    Region glu_part, glu_part2, de0, wg_part, gemm_part;
    Region xch[2], epoch[2];
    size_t total;
};
static GWs make_gws(const Geo& g) {
    GWs W;
    RegionCursor put;
    const size_t C = g.C, H = g.H, bt = (size_t)g.B * g.T3;
    const size_t n0 = (size_t)g.B * g.H1 * g.W1 * C, n1 = (size_t)g.B * g.H2 * g.W2 * C;
    put(W.d_out, bt * 2 * H * 4);
    for (int l = 0; l < 2; ++l) { put(W.dgi[l], bt * 6 * H * 4); put(W.dgh[l], bt * 6 * H * 4); put(W.hprev[l], bt * 2 * H * 4); }
    put(W.d_in, 2 * bt * 2 * H * 4);          // (H = 64: two direction planes, gru4.hip; generic: one tensor)
    put(W.heads_part, heads_part_floats(g.B, g.T3, g.NC, 2 * H) * 4);
    const size_t E = esz(g);
    put(W.dp[2], 2 * bt * C * 4); put(W.dz[2], n1 * E); put(W.dp[1], n1 * E); put(W.dz[1], n0 * E); put(W.dp[0], n0 * E);
    put(W.coef[1], 3 * C * 4); put(W.coef[2], 3 * C * 4);
    put(W.glu_part, (size_t)(g.mode == SED_DTYPE_BF16 ? bglu_bwd_grid(g.C, g.B, g.H1, g.W1) : gglu_bwd_grid(g.B, g.H1, g.W1)) * (C * C + 3 * C) * 4);
    put(W.glu_part2, (size_t)GPART_SLICES * (C * C + 3 * C) * 4);
    put(W.de0, 2 * C * 10 * sizeof(double));
    put(W.wg_part, (size_t)gwgrad_slabs(g.C) * 9 * C * C * 4);
    put(W.gemm_part, 2 * gru_gemm_part_floats(g) * 4);     // one per GRU layer: their batches may overlap in time
    for (int l = 0; l < 2; ++l) { put(W.xch[l], g.H == 256 ? gclu_xch_bytes(g.B, g.H, 1) : 0); put(W.epoch[l], (size_t)2 * g.B * 4); }
    W.total = put.o;
    return W;
}

size_t gen_ctx_bytes(const Geo& g) { return make_gctx(g).total; }
size_t gen_ws_bytes(const Geo& g) { return make_gws(g).total; }

int gen_ctx_view(const Geo& g, const char* name, size_t* offset, size_t* bytes) {
    const GCtx L = make_gctx(g);
    struct { const char* n; Region r; } tab[] = {
        {"mom0", L.mom0}, {"bn0", L.bn[0]}, {"p0", L.p[0]}, {"y1", L.y[1]}, {"stat1", L.stat[1]}, {"bn1", L.bn[1]}, {"p1", L.p[1]},
        {"y2", L.y[2]}, {"stat2", L.stat[2]}, {"bn2", L.bn[2]}, {"p2", L.p[2]}, {"gates0", L.gates[0]}, {"gates1", L.gates[1]},
        {"gru0", L.out[0]}, {"gru1", L.out[1]}, {"logits_s", L.logits_s}, {"den", L.den_sv},
        {"gru_err", L.err.sub(0, 4)},         // (the counter; its region is a whole 256-byte line)
    };
    for (auto& t : tab)
        if (strcmp(t.n, name) == 0) { *offset = t.r.off; *bytes = t.r.bytes; return SED_OK; }
    sed_set_error("sed_crnn_ctx_view: unknown buffer '%s'", name);
    return SED_ERR_BAD_ARG;
}

// Regions the library needs INITIALISED before the first forward / backward on a fresh buffer (everything else is written
// before it is read): the cluster recurrence's exchange granules + launch epochs (a stale word that happened to carry a
// matching tag would be consumed as a fresh value) and the sticky spin-timeout counter.
int gen_buffers_init(const Geo& g, void* ctx, size_t ctx_bytes, void* ws, size_t ws_bytes, hipStream_t st) {
    if (ctx) {
        const GCtx L = make_gctx(g);
        if (ctx_bytes < L.total) { sed_set_error("sed_crnn_buffers_init: ctx has %zu bytes, needs %zu", ctx_bytes, L.total); return SED_ERR_WORKSPACE; }
        // xch[0] .. err are laid out back to back apart from the small per-layer W_ih transposes: clear each piece
        for (int l = 0; l < 2; ++l) {
            if (L.xch[l].bytes) SED_CHECK_HIP(hipMemsetAsync(L.xch[l].v(ctx), 0, L.xch[l].bytes, st));
            SED_CHECK_HIP(hipMemsetAsync(L.epoch[l].v(ctx), 0, L.epoch[l].bytes, st));
        }
        SED_CHECK_HIP(hipMemsetAsync(L.err.v(ctx), 0, L.err.bytes, st));
    }
    if (ws) {
        const GWs W = make_gws(g);
        if (ws_bytes < W.total) { sed_set_error("sed_crnn_buffers_init: ws has %zu bytes, needs %zu", ws_bytes, W.total); return SED_ERR_WORKSPACE; }
        for (int l = 0; l < 2; ++l) {
            if (W.xch[l].bytes) SED_CHECK_HIP(hipMemsetAsync(W.xch[l].v(ws), 0, W.xch[l].bytes, st));
            SED_CHECK_HIP(hipMemsetAsync(W.epoch[l].v(ws), 0, W.epoch[l].bytes, st));
        }
    }
    return SED_OK;
}

// the recurrent tail's buffers in the generic layouts (ws == null: a forward)
static RnnBufs rnn_bufs(const Geo& g, const GCtx& L, void* ctx, const GWs* Wp, void* ws) {
    RnnBufs R;
    R.p2 = L.p[2].f(ctx);
    R.logits_s = L.logits_s.f(ctx); R.strong_sv = L.strong_sv.f(ctx); R.weak_sv = L.weak_sv.f(ctx); R.den_sv = L.den_sv.f(ctx);
    R.err = (int*)L.err.v(ctx);
    for (int l = 0; l < 2; ++l) {
        R.out[l] = L.out[l].f(ctx); R.gates[l] = L.gates[l].f(ctx);
        R.gi[l] = L.gi[l].f(ctx); R.wihT[l] = L.wihT[l].f(ctx); R.whh[l] = L.whh[l].v(ctx); R.whhT[l] = L.whhT[l].v(ctx);
        R.xch[l] = ws ? Wp->xch[l].v(ws) : L.xch[l].v(ctx);
        R.epoch[l] = (unsigned int*)(ws ? Wp->epoch[l].v(ws) : L.epoch[l].v(ctx));
    }
    if (ws == nullptr) return R;
    const GWs& W = *Wp;
    R.d_out = W.d_out.f(ws); R.d_in = W.d_in.f(ws); R.dp2 = W.dp[2].f(ws); R.heads_part = W.heads_part.f(ws);
    for (int l = 0; l < 2; ++l) { R.dgi[l] = W.dgi[l].f(ws); R.dgh[l] = W.dgh[l].f(ws); R.hprev[l] = W.hprev[l].f(ws); }
    R.gemm_part = W.gemm_part.f(ws); R.gemm_part_floats = R.gemm_part_stride = gru_gemm_part_floats(g); R.splitk = gru_splitk(g);
    R.zero = W.de0.d(ws); R.n_zero = (int)(W.de0.bytes / sizeof(double));
    return R;
}

int gen_mompart(const Geo& g, void* ctx, size_t ctx_bytes, double** out) {
    const GCtx L = make_gctx(g);
    if (ctx_bytes < L.total) {
        sed_set_error("sed_crnn_moments: ctx has %zu bytes, needs %zu", ctx_bytes, L.total);
        return SED_ERR_WORKSPACE;
    }
    *out = L.mompart.d(ctx);
    return SED_OK;
}

int gen_forward(const Geo& g, const ParamOff& P, const float* params, float* bn_running, int64_t* bn_tracked, const float* x,
                int train, int update_bn, const uint64_t* seed_dev, void* ctx, size_t ctx_bytes, float* strong, float* weak,
                hipStream_t st) {
    const int mom_ready = (train & 4) ? 1 : 0;      // (sed_crnn_forward's train bit 2)
    train &= 3;
    const GCtx L = make_gctx(g);
    if (ctx_bytes < L.total) {
        sed_set_error("sed_crnn_forward: ctx has %zu bytes, needs %zu", ctx_bytes, L.total);
        return SED_ERR_WORKSPACE;
    }
    const int C = g.C, H = g.H;
    const int use_drop = (train && g.p > 0.f) ? 1 : 0;
    const int upd = (train && update_bn) ? 1 : 0;
    // train & 2: train-mode arithmetic, but no backward will ever run on this ctx (the teacher's forward, main.py:87-89): what only
    // a backward reads need not be written - today the bf16 activation copies of SED_DTYPE_F16
    const bool keep_b16 = train && !(train & 2);
    int64_t* trk[3] = {bn_tracked ? bn_tracked + 0 : nullptr, bn_tracked ? bn_tracked + 1 : nullptr,
                       bn_tracked ? bn_tracked + 2 : nullptr};
    // ---- weight packing (conv panels, GLU weights folded with the BatchNorm affine, GRU streaming layout) + the fp64
    //      BatchNorm accumulators of blocks 1 and 2 ----------------------------------------------------------------------
    GenPackArgs pk = {};
    pk.C = C;
    pk.w1 = params + P.conv_w[1]; pk.w2 = params + P.conv_w[2];
    pk.wpk1 = L.wpk[1].v(ctx); pk.wpk2 = L.wpk[2].v(ctx);
    pk.wpkT1 = train ? L.wpkT[1].v(ctx) : nullptr; pk.wpkT2 = train ? L.wpkT[2].v(ctx) : nullptr;
    pk.glu_w1 = params + P.glu_w[1]; pk.glu_w2 = params + P.glu_w[2]; pk.glu_b1 = params + P.glu_b[1]; pk.glu_b2 = params + P.glu_b[2];
    pk.gamma1 = params + P.bn_g[1]; pk.gamma2 = params + P.bn_g[2]; pk.beta1 = params + P.bn_b[1]; pk.beta2 = params + P.bn_b[2];
    pk.wg1 = L.wg[1].v(ctx); pk.wg2 = L.wg[2].v(ctx);
    pk.wgT1 = train ? L.wgT[1].v(ctx) : nullptr; pk.wgT2 = train ? L.wgT[2].v(ctx) : nullptr;
    pk.bg1 = L.bg[1].f(ctx); pk.bg2 = L.bg[2].f(ctx);
    pk.zero = L.stat[1].d(ctx); pk.n_zero = train ? 4 * C : 0;
    pk.f16 = g.f16 ? 1 : 0;
    // (The packing is independent of block 0, but forking it onto the helper stream is not an option: a forward that
    // itself runs on a forked stream - the teacher's, next to the student's - would fork a second time inside the same
    // hipGraph capture, and ROCm 7.0's hipStreamEndCapture segfaults on that nested fork.  It stays on the caller's stream.)
    // Training forwards: the packing and the W_ih transposes ride in spare workgroups of block 0's moments launch (gpack.h).
    // Eval forwards have no moments launch and need no transposes.
    const bool aux_pack = train != 0;
    GenAuxPack aux = {};
    if (aux_pack) {
        aux.pk = pk; aux.mode = g.mode; aux.n_gnt = 0;
        if (H != 64)
            for (int l = 0; l < g.L && l < 2; ++l) {
                aux.gw0[l] = params + P.w_ih[l][0]; aux.gw1[l] = params + P.w_ih[l][1]; aux.gout[l] = L.wihT[l].f(ctx);
                aux.gR[l] = 3 * H; aux.gN[l] = (l == 0) ? C : 2 * H;
                aux.n_gnt = l + 1;
            }
        // the W_hh layouts of the one-CU bf16 recurrence too (k_grec_pack: 6 us in front of every recurrence launch)
        if (H == 256 && g.mode == SED_DTYPE_BF16)
            for (int l = 0; l < g.L && l < 2; ++l) {
                aux.rw0[l] = params + P.w_hh[l][0]; aux.rw1[l] = params + P.w_hh[l][1];
                aux.rwp[l] = L.whh[l].v(ctx); aux.rwpT[l] = L.whhT[l].v(ctx);
                aux.n_grec = l + 1;
            }
    } else {
        SED_TRY(launch_gen_pack(pk, g.mode, st));
    }

    // ---- conv block 0 -------------------------------------------------------------------------------------------------
    SED_TRY(launch_blk0_forward(g, x, params + P.conv_w[0], params + P.conv_b[0], params + P.bn_g[0], params + P.bn_b[0],
                                params + P.glu_w[0], params + P.glu_b[0], bn_running + 0, bn_running + C, trk[0], train, upd,
                                seed_dev, L.mom0.d(ctx), L.mompart.d(ctx), L.wz0.f(ctx), L.wl0.f(ctx), L.bn[0].f(ctx),
                                g.f16 ? L.ph[0].f(ctx) : L.p[0].f(ctx),
                                use_drop ? L.mask[0].m(ctx) : nullptr, nullptr, st, 0, aux_pack ? &aux : nullptr,
                                (g.f16 && keep_b16) ? L.p[0].v(ctx) : nullptr, mom_ready));
    // ---- conv blocks 1, 2 -----------------------------------------------------------------------------------------------
    const int Hs[3] = {0, g.H1, g.H2}, Wd[3] = {0, g.W1, g.W2};
    auto bn_args = [&](int i) {
        GBnArgs bn;
        bn.stat = L.stat[i].d(ctx); bn.N = (double)g.B * Hs[i] * Wd[i]; bn.gamma = params + P.bn_g[i]; bn.beta = params + P.bn_b[i];
        bn.run_mean = bn_running + (2 * i) * C; bn.run_var = bn_running + (2 * i + 1) * C; bn.tracked = trk[i];
        bn.train = train; bn.update = upd; bn.eps = g.eps; bn.momentum = g.mom; bn.bn = L.bn[i].f(ctx);
        return bn;
    };
    for (int i = 1; i <= 2; ++i) {
        const GBnArgs bn = bn_args(i);
        if (g.f16) {
            // SED_DTYPE_F16: the forward chain runs on the fp16 tensors ph / yh; a training forward also leaves the bf16 copies
            // y[i] / p[i] that the (bf16-family) backward kernels read
            SED_TRY(launch_bconv_fwd(2, C, L.ph[i - 1].v(ctx), L.wpk[i].v(ctx), params + P.conv_b[i], L.yh[i].v(ctx),
                                     train ? L.stat[i].d(ctx) : nullptr, g.B, Hs[i], Wd[i], st));
            SED_TRY(launch_bglu_fwd(C, L.yh[i].v(ctx), bn, params + P.glu_w[i], params + P.glu_b[i], i == 1 ? L.ph[1].v(ctx) : L.p[2].v(ctx),
                                    i == 1 ? 1 : 0, g.B, Hs[i], Wd[i], i, use_drop, g.p, seed_dev, use_drop ? L.mask[i].m(ctx) : nullptr,
                                    train ? L.wg[i].v(ctx) : nullptr, train ? L.bg[i].f(ctx) : nullptr, st, 1,
                                    (i == 1 && keep_b16) ? L.p[1].v(ctx) : nullptr, keep_b16 ? L.y[i].v(ctx) : nullptr));
            continue;
        }
        if (g.mode != SED_DTYPE_F32)      // bf16 (bf16 storage) / bf16x3 (fp32 storage, split operands): bconv.hip
            SED_TRY(launch_bconv_fwd(g.mode == SED_DTYPE_BF16X3, C, L.p[i - 1].v(ctx), L.wpk[i].v(ctx), params + P.conv_b[i], L.y[i].v(ctx),
                                     train ? L.stat[i].d(ctx) : nullptr, g.B, Hs[i], Wd[i], st));
        else
            SED_TRY(launch_gconv_fwd(C, L.p[i - 1].f(ctx), L.wpk[i].v(ctx), params + P.conv_b[i], L.y[i].f(ctx),
                                     train ? L.stat[i].d(ctx) : nullptr, g.B, Hs[i], Wd[i], st));
        if (g.mode == SED_DTYPE_BF16)
            SED_TRY(launch_bglu_fwd(C, L.y[i].v(ctx), bn, params + P.glu_w[i], params + P.glu_b[i], L.p[i].v(ctx), i == 1 ? 1 : 0, g.B,
                                    Hs[i], Wd[i], i, use_drop, g.p, seed_dev, use_drop ? L.mask[i].m(ctx) : nullptr,
                                    train ? L.wg[i].v(ctx) : nullptr, train ? L.bg[i].f(ctx) : nullptr, st));
        else if (g.mode == SED_DTYPE_BF16X3)
            SED_TRY(launch_bglu_fwd_x3(C, L.y[i].v(ctx), bn, params + P.glu_w[i], params + P.glu_b[i], L.p[i].v(ctx), g.B, Hs[i], Wd[i], i,
                                       use_drop, g.p, seed_dev, use_drop ? L.mask[i].m(ctx) : nullptr, st));
        else
            SED_TRY(launch_gglu_fwd(C, L.y[i].v(ctx), bn, L.wg[i].v(ctx), L.bg[i].f(ctx), L.p[i].v(ctx), g.B, Hs[i], Wd[i], i, use_drop, g.p,
                                    seed_dev, use_drop ? L.mask[i].m(ctx) : nullptr, st));
    }
    // ---- BiGRU + heads ---------------------------------------------------------------------------------------------------
    return rnn_forward(g, P, params, rnn_bufs(g, L, ctx, nullptr, nullptr), train, seed_dev, strong, weak, aux.n_grec, st);
}

// Backward.  `side`: the helper stream of the caller's stream (owned by crnn.hip), or the caller's own.
int gen_backward(const Geo& g, const ParamOff& P, const float* params, const float* x, const uint64_t* seed_dev, void* ctx,
                 size_t ctx_bytes, const float* d_strong, const float* d_weak, float* grads, void* ws, size_t ws_bytes, int parts,
                 hipStream_t st, SideFork& side, const HeadsLoss* hl, const HeadsOut* ho, const float* d_att) {
    const GCtx L = make_gctx(g);
    const GWs W = make_gws(g);
    if (ctx_bytes < L.total || ws_bytes < W.total) {
        sed_set_error("sed_crnn_backward: ctx %zu/%zu bytes, ws %zu/%zu bytes", ctx_bytes, L.total, ws_bytes, W.total);
        return SED_ERR_WORKSPACE;
    }
    const int C = g.C, H = g.H, BT = g.B * g.T3;
    const int use_drop = (g.p > 0.f) ? 1 : 0;
    // ---- heads, BiGRU (+ the weight-gradient tail of a parts == 1 / parts == 8 call) ------------------------------------------
    const RnnBwd rb = rnn_backward_plan(g, P, rnn_bufs(g, L, ctx, &W, ws), params, grads, seed_dev, hl, ho, parts, &side, d_att);
    SED_TRY(rnn_backward(rb, d_strong, d_weak, st));
    if (!(parts & 2)) return SED_OK;
    // ---- conv blocks 2, 1 -------------------------------------------------------------------------------------------------
    if (!(parts & 1)) SED_CHECK_HIP(hipMemsetAsync(W.de0.d(ws), 0, W.de0.bytes, st));
    const int Hs[3] = {0, g.H1, g.H2}, Wd[3] = {0, g.W1, g.W2};
    for (int i = 2; i >= 1; --i) {
        // (H = 64: the GRU's dX arrives as two direction planes; the GLU backward adds them while loading)
        const float* dp2 = (i == 2 && H == 64) ? W.dp[2].f(ws) + (size_t)BT * C : nullptr;
        const bool bf16_glu = g.mode == SED_DTYPE_BF16;      // bglu.hip (bf16 storage); fp32 and bf16x3: gglu.hip
        if (bf16_glu)
            SED_TRY(launch_bglu_bwd(C, L.y[i].v(ctx), L.bn[i].f(ctx), L.wg[i].v(ctx), L.bg[i].f(ctx), L.wgT[i].v(ctx), W.dp[i].f(ws), i == 1 ? 1 : 0,
                                    W.dz[i].f(ws), W.glu_part.f(ws), g.B, Hs[i], Wd[i], use_drop, g.p, L.mask[i].m(ctx), st, dp2));
        else
            SED_TRY(launch_gglu_bwd(C, L.y[i].v(ctx), L.bn[i].f(ctx), params + P.bn_g[i], params + P.bn_b[i], L.wg[i].v(ctx), L.wgT[i].v(ctx),
                                    L.bg[i].f(ctx), W.dp[i].f(ws), W.dz[i].f(ws), W.glu_part.f(ws), g.B, Hs[i], Wd[i], use_drop, g.p,
                                    L.mask[i].m(ctx), st, dp2));
        GBnBwdArgs pa;
        pa.part = W.glu_part.f(ws); pa.n_part = bf16_glu ? bglu_bwd_grid(C, g.B, Hs[i], Wd[i]) : gglu_bwd_grid(g.B, Hs[i], Wd[i]); pa.C = C; pa.N = (double)g.B * Hs[i] * Wd[i];
        pa.part2 = W.glu_part2.f(ws);
        pa.gamma = params + P.bn_g[i]; pa.beta = params + P.bn_b[i]; pa.bn = L.bn[i].f(ctx); pa.coef = W.coef[i].f(ws);
        pa.g_gamma = grads + P.bn_g[i]; pa.g_beta = grads + P.bn_b[i]; pa.g_wglu = grads + P.glu_w[i]; pa.g_bglu = grads + P.glu_b[i];
        pa.g_convb = grads + P.conv_b[i];
        SED_TRY(launch_gbn_bwd_prep(pa, st));
        // The weight gradient (helper stream) and the data gradient (caller's stream) both depend on the coefficients only; the
        // data gradient - the critical chain - is captured between the two halves of the fork (SideFork)
        SED_TRY(side.mark(st));
        if (g.mode != SED_DTYPE_F32)
            SED_TRY(launch_bconv_dgrad(g.mode == SED_DTYPE_BF16X3, C, W.dz[i].f(ws), L.y[i].v(ctx), W.coef[i].f(ws), L.wpkT[i].v(ctx),
                                       W.dp[i - 1].f(ws), g.B, Hs[i], Wd[i], st));
        else
            SED_TRY(launch_gconv_dgrad(C, W.dz[i].f(ws), L.y[i].f(ctx), W.coef[i].f(ws), L.wpkT[i].v(ctx), W.dp[i - 1].f(ws), g.B, Hs[i], Wd[i],
                                       st));
        SED_TRY(side.start());
        SED_TRY(launch_gwgrad(g.mode, C, W.dz[i].f(ws), L.y[i].f(ctx), W.coef[i].f(ws), L.p[i - 1].f(ctx), W.wg_part.f(ws), grads + P.conv_w[i], g.B,
                              Hs[i], Wd[i], side.s));
        if (i == 2) SED_TRY(rnn_deferred_weight_grads(rb));      // parts == 3, H = 64: head column sum + GRU dW / db behind wgrad2
    }
    // ---- conv block 0 -----------------------------------------------------------------------------------------------------
    SED_TRY(launch_blk0_backward(g, x, params + P.conv_w[0], params + P.conv_b[0], params + P.bn_g[0], params + P.bn_b[0],
                                 params + P.glu_w[0], L.mask[0].m(ctx), L.mom0.d(ctx), L.wz0.f(ctx), L.wl0.f(ctx), L.bn[0].f(ctx), W.dp[0].f(ws),
                                 W.de0.d(ws), 0, grads + P.conv_w[0], grads + P.conv_b[0], grads + P.bn_g[0], grads + P.bn_b[0],
                                 grads + P.glu_w[0], grads + P.glu_b[0], st));
    return side.join(st);
}


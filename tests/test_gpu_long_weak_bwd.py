"""-m gpu tests of training on recording-level tags: sed_stitch_weak_backward against the float64 statement
(tests/weak_bwd_np.py), its closed form on one full window, error bits, bad arguments, reproducibility and graph replay;
sed_crnn_backward_att against sed_crnn_backward (NULL attention gradient: bit-identical; the weak tag's own gradient routed
through d_strong / d_att: equal to rounding), against the float64 oracle and in the f16 mode against fp32; and one backward plus
three Adam steps of train.train_recording_tags against float64 autograd through the oracle.  Every buffer a kernel writes
starts as 0xFF bytes and carries a tail that must come back untouched."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu, synth
from tests import gpu_util as gu
from tests import weak_bwd_np, weak_np
from tests.long_util import SENT, TAIL, _Scaler, _tables, _tile
from tests.test_gpu_generic import F16_GRAD_TOL, _grad_errors
from tests.test_gpu_long import _recordings
from tests.test_gpu_long_weak import WeakCall
from tests.test_gpu_parity import _check_grads

pytestmark = pytest.mark.gpu

NAMES = ("p", "a", "ds", "da")


def _step32(got, want):
    """Distance in float32 steps between two float32 arrays of finite values of any sign."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(got) - key(want))


class BwdCall:
    """One sed_stitch_weak_backward call: the forward's sums come from the GPU (WeakCall), both outputs start as 0xFF bytes with
    a tail of TAIL floats, a second error word.  ``misalign``: one of "p", "a", "ds", "da" shifts that tensor off 16 bytes."""

    def __init__(self, p, a, rec_win0, rec_frame0, hop3, weighting, g, misalign=None):
        from dcase2019_task4_amd import _lib
        self._lib, self.l = _lib, _lib.lib()
        p, a = np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(a, dtype=np.float32)
        self.n_win, self.T3, self.NC = p.shape
        self.n_rec, self.hop3, self.weighting = len(rec_win0) - 1, int(hop3), int(weighting)
        self.n = p.size
        fwd = WeakCall(p, a, rec_win0, rec_frame0, hop3, weighting).run()
        self.fwd_err, self.sums_host = fwd["err"], fwd["sums"]
        self.sums = torch.from_numpy(np.ascontiguousarray(fwd["sums"])).cuda()
        self.g = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda()
        self._bufs = {}
        for name, src in (("p", p), ("a", a), ("ds", None), ("da", None)):
            off = 1 if misalign == name else 0
            buf = torch.empty(off + self.n + TAIL, dtype=torch.float32, device="cuda")
            assert (buf[off:].data_ptr() % 16 != 0) == bool(off)
            if src is not None:
                buf[off:off + self.n].copy_(torch.from_numpy(src.reshape(-1)))
            self._bufs[name] = buf
            setattr(self, name, buf[off:])
        self.rec_win0 = torch.from_numpy(np.asarray(rec_win0, dtype=np.int32)).cuda()
        self.rec_frame0 = torch.from_numpy(np.asarray(rec_frame0, dtype=np.int64)).cuda()
        self.err = torch.empty(2, dtype=torch.int32, device="cuda")

    def fill(self):
        for name in ("ds", "da"):
            getattr(self, name).view(torch.int32).fill_(-1)          # 0xFF bytes
        self.err.fill_(SENT)
        self.err[:1].zero_()

    def launch(self, **kw):
        ptr = self._lib.ptr
        k = dict(p=self.p, a=self.a, n_rec=self.n_rec, T3=self.T3, NC=self.NC, hop3=self.hop3, weighting=self.weighting,
                 sums=self.sums, g=self.g, ds=self.ds, da=self.da, err=self.err, w0=self.rec_win0, f0=self.rec_frame0)
        k.update(kw)
        return self.l.sed_stitch_weak_backward(ptr(k["p"]), ptr(k["a"]), ptr(k["w0"]), ptr(k["f0"]), k["n_rec"], k["T3"], k["NC"],
                                               k["hop3"], k["weighting"], ptr(k["sums"]), ptr(k["g"]), ptr(k["ds"]), ptr(k["da"]),
                                               ptr(k["err"]), self._lib.stream_ptr())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.ds.view(torch.int32) == -1).all() and (self.da.view(torch.int32) == -1).all()
                    and int(self.err[0].item()) == 0 and int(self.err[1].item()) == SENT)

    def get(self):
        torch.cuda.synchronize()
        out = {}
        for name in ("ds", "da"):
            t = getattr(self, name)
            assert (t[self.n:].view(torch.int32) == -1).all(), name
            out[name] = t[:self.n].cpu().numpy().reshape(self.n_win, self.T3, self.NC)
        assert int(self.err[1].item()) == SENT
        out["err"] = int(self.err[0].item())
        return out

    def run(self):
        self.fill()
        assert self.launch() == 0, self.l.sed_last_error()
        return self.get()


def _inputs(rs, n_win, T3, NC):
    return rs.uniform(size=(n_win, T3, NC)).astype(np.float32), weak_np.attention(rs, n_win, T3, NC)


def _g(rs, n_rec, NC):
    g = rs.standard_normal((n_rec, NC)).astype(np.float32)
    g[rs.uniform(size=g.shape) < 0.15] = 0.0
    g[0, 0] = 0.0
    return g


def _check(got, want, what):
    """Every element within one float32 step of the statement (the same fp64 operations in the same order; the step is for a
    last-bit difference in an fp64 division); where the statement is +0.0, +0.0 bit for bit unless a zero gradient made it so."""
    n_diff = 0
    for name, w in zip(("ds", "da"), want):
        assert not np.isnan(got[name]).any(), (what, name)
        d = _step32(got[name], w)
        assert (d <= 1).all(), (what, name, int(d.max()))
        n_diff += int((d != 0).sum())
    print(f"{what}: {n_diff} of {2 * got['ds'].size} elements not bit-equal to the statement")


def _tails_are_plus_zero(got, rec_win0, rec_frame0, T3, hop3):
    zero = np.zeros(got["ds"].shape[2], np.float32).tobytes()
    n = 0
    for r in range(len(rec_win0) - 1):
        L3 = int(rec_frame0[r + 1] - rec_frame0[r])
        for j in range(int(rec_win0[r + 1] - rec_win0[r])):
            for v in range(max(0, L3 - j * hop3), T3):
                assert got["ds"][rec_win0[r] + j, v].tobytes() == zero and got["da"][rec_win0[r] + j, v].tobytes() == zero, (r, j, v)
                n += 1
    return n


# ---- the kernel against the statement ------------------------------------------------------------------------------------------
_REF = {}


@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", [1, 3, 8])
@pytest.mark.parametrize("NC,misalign", [(1, None), (3, None), (10, None), (12, None), (12, "p"), (12, "a"), (12, "ds"), (12, "da")])
def test_gradients_match_the_float64_statement(NC, misalign, hop3, weighting):
    T3 = 8
    L3s = [1, 5, 8, 9, 23, 2 * _tile() + 5]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    seed = 2000 + 100 * NC + 10 * hop3 + weighting
    rs = np.random.RandomState(seed)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    g = _g(rs, len(L3s), NC)
    assert (a == np.float32(1.0)).any() and (NC == 1 or (a == np.float32(1e-7)).any()) and (g == 0).any()
    call = BwdCall(p, a, rec_win0, rec_frame0, hop3, weighting, g, misalign=misalign)
    got = call.run()
    assert call.fwd_err == 0 and got["err"] == 0
    if seed not in _REF:                               # (the misaligned cases share the aligned case's inputs and sums)
        _REF.clear()
        _REF[seed] = weak_bwd_np.backward(p, a, rec_win0, rec_frame0, hop3, weighting, g, sums=call.sums_host)
    _check(got, _REF[seed], f"NC={NC} misalign={misalign} hop3={hop3} weighting={weighting}")
    assert _tails_are_plus_zero(got, rec_win0, rec_frame0, T3, hop3) > 0
    if misalign is not None:                           # the 16-byte path and the scalar path: identical bytes
        aligned = BwdCall(p, a, rec_win0, rec_frame0, hop3, weighting, g).run()
        assert aligned["ds"].tobytes() == got["ds"].tobytes() and aligned["da"].tobytes() == got["da"].tobytes()


@pytest.mark.parametrize("NC", [3, 12])
def test_one_full_window_gives_the_closed_form(NC):
    """A recording of exactly one full window: w / W = 1, d_win_strong = g A / den and d_win_att = g (P - t) / den, from the
    window's own values and the forward's sums; and sum_v d_win_strong = g (the attention-weighted mean passes a uniform shift)
    up to the float32 rounding of the T3 terms."""
    T3 = 8
    rec_win0, rec_frame0 = _tables([T3, T3, T3], T3, 4)
    rs = np.random.RandomState(80 + NC)
    p, a = _inputs(rs, 3, T3, NC)
    g = _g(rs, 3, NC)
    call = BwdCall(p, a, rec_win0, rec_frame0, 4, 1, g)
    got = call.run()
    assert got["err"] == 0
    num, den = call.sums_host[:, None, :, 0], call.sums_host[:, None, :, 1]
    g64 = g.astype(np.float64)[:, None, :]
    want_s = (g64 * a.astype(np.float64) / den).astype(np.float32)
    want_a = (g64 * (p.astype(np.float64) - num / den) / den).astype(np.float32)
    assert (_step32(got["ds"], want_s) <= 1).all() and (_step32(got["da"], want_a) <= 1).all()
    np.testing.assert_allclose(got["ds"].astype(np.float64).sum(1), g, rtol=0, atol=T3 * 2.0 ** -24 * np.abs(g).max())


# ---- error paths -------------------------------------------------------------------------------------------------------------------
def _check_valid_and_zero(call, got, p, a, g, valid, hop3, n_win):
    """Every recording of `valid` = {r: (w0, nw, L3)} has the statement's gradients on that recording alone; every other window is
    +0.0 bit for bit."""
    zero = np.zeros(p.shape[1:], np.float32).tobytes()
    owned = set()
    for r, (w0, nw, L3) in valid.items():
        want = weak_bwd_np.backward(p[w0:w0 + nw], a[w0:w0 + nw], [0, nw], [0, L3], hop3, 0, g[r:r + 1], sums=call.sums_host[r:r + 1])
        _check({"ds": got["ds"][w0:w0 + nw], "da": got["da"][w0:w0 + nw]}, want, f"row {r}")
        owned.update(range(w0, w0 + nw))
    for w in range(n_win):
        if w not in owned:
            assert got["ds"][w].tobytes() == zero and got["da"][w].tobytes() == zero, w


def test_too_few_windows_raise_bit_32_and_those_windows_are_zero():
    """Recording 1 needs 4 windows and is given 2."""
    T3, NC = 8, 3
    rs = np.random.RandomState(90)
    p, a = _inputs(rs, 4, T3, NC)
    g = _g(rs, 3, NC)
    call = BwdCall(p, a, [0, 1, 3, 4], [0, 8, 38, 46], T3, 0, g)
    got = call.run()
    assert call.fwd_err == 32 and got["err"] == 32
    _check_valid_and_zero(call, got, p, a, g, {0: (0, 1, 8), 2: (3, 1, 8)}, T3, 4)


@pytest.mark.parametrize("rec_win0,rec_frame0,valid,n_win", [
    ([0, 3, 4, 6], [0, 20, 16, 30], {0: (0, 3, 20), 2: (4, 2, 14)}, 6),      # frames run backwards
    ([0, 1, 9, 3], [0, 8, 16, 24], {0: (0, 1, 8)}, 3),                       # windows beyond the table's own total
    ([0, 2, 2, 4], [0, 16, 16, 30], {0: (0, 2, 16), 2: (2, 2, 14)}, 4),      # an empty recording
])
def test_malformed_tables_raise_bit_16_and_those_windows_are_zero(rec_win0, rec_frame0, valid, n_win):
    T3, NC = 8, 3
    rs = np.random.RandomState(91)
    p, a = _inputs(rs, 6, T3, NC)
    g = _g(rs, 3, NC)
    call = BwdCall(p, a, rec_win0, rec_frame0, T3, 0, g)
    got = call.run()
    assert got["err"] & 16 and not got["err"] & ~48 and got["err"] == call.fwd_err
    _check_valid_and_zero(call, got, p, a, g, valid, T3, n_win)
    # beyond rec_win0[n_rec] nothing is written: the call owns [0, n_win) only
    assert (call.ds[n_win * T3 * NC:].view(torch.int32) == -1).all() and (call.da[n_win * T3 * NC:].view(torch.int32) == -1).all()


def test_a_total_outside_the_limits_raises_bit_16_and_every_window_is_zero():
    T3, NC = 8, 3
    rs = np.random.RandomState(92)
    p, a = _inputs(rs, 2, T3, NC)
    call = BwdCall(p, a, [0, 1, 2], [0, 8, 16], T3, 0, _g(rs, 2, NC))
    for total in (0, -5, 2 ** 31 // NC + 1, 2 ** 40):
        call.fill()
        assert call.launch(f0=torch.tensor([0, 8, total], dtype=torch.int64, device="cuda")) == 0
        got = call.get()
        assert got["err"] == 16, total
        assert not got["ds"].view(np.int32).any() and not got["da"].view(np.int32).any(), total


def test_bad_host_arguments_return_bad_arg_before_any_launch():
    T3, NC = 8, 3
    rec_win0, rec_frame0 = _tables([8, 20], T3, T3)
    rs = np.random.RandomState(93)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    call = BwdCall(p, a, rec_win0, rec_frame0, T3, 0, _g(rs, 2, NC))
    call.fill()
    for kw in (dict(NC=17), dict(NC=0), dict(hop3=0), dict(hop3=9), dict(T3=0), dict(T3=4097, hop3=1), dict(weighting=2),
               dict(n_rec=0), dict(p=None), dict(a=None), dict(w0=None), dict(f0=None), dict(sums=None), dict(g=None), dict(ds=None),
               dict(da=None), dict(err=None)):
        assert call.launch(**kw) == -1, kw                                       # SED_ERR_BAD_ARG
    assert call.untouched()
    assert call.launch() == 0
    assert call.get()["err"] == 0


def test_two_calls_and_a_graph_replay_give_identical_bytes():
    T3, NC, hop3 = 8, 10, 3
    L3s = [3 * _tile() + 9, 5, 40]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    rs = np.random.RandomState(94)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    call = BwdCall(p, a, rec_win0, rec_frame0, hop3, 1, _g(rs, 3, NC))
    first = call.run()
    second = call.run()
    assert first["err"] == 0 and first["ds"].any() and first["da"].any()
    graph = torch.cuda.CUDAGraph()
    call.fill()
    with torch.cuda.graph(graph):
        assert call.launch() == 0
    call.fill()
    graph.replay()
    third = call.get()
    for other in (second, third):
        assert other["err"] == 0
        assert first["ds"].tobytes() == other["ds"].tobytes() and first["da"].tobytes() == other["da"].tobytes()


# ---- the autograd node -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NC", [10, 12])
def test_pooled_tags_backward_gives_the_bytes_of_the_direct_call(NC):
    from dcase2019_task4_amd.inference import pooled_tags, stitch_weak
    T3, hop3 = 8, 3
    L3s = [_tile() + 9, 5, 40]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    rs = np.random.RandomState(211 + NC)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    tp, ta = torch.from_numpy(p).cuda().requires_grad_(True), torch.from_numpy(a).cuda().requires_grad_(True)
    w0, f0 = torch.from_numpy(rec_win0).cuda(), torch.from_numpy(rec_frame0).cuda()
    weak, err = pooled_tags(tp, ta, w0, f0, int(rec_frame0[-1]), hop3, n_win=int(rec_win0[-1]))
    plain = stitch_weak(tp.detach(), ta.detach(), w0, f0, int(rec_frame0[-1]), hop3, want_sums=True)
    assert weak.requires_grad and torch.equal(weak.detach(), plain["weak"])
    g = rs.standard_normal((len(L3s), NC)).astype(np.float32)
    weak.backward(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    assert int(err.item()) == 0 and int(plain["err"].item()) == 0
    call = BwdCall(p, a, rec_win0, rec_frame0, hop3, 1, g)
    call.sums = plain["sums"]                                                    # stitch_weak's own sums, not the helper's forward
    want = call.run()
    assert want["err"] == 0 and want["ds"].any() and want["da"].any()
    assert tp.grad.cpu().numpy().tobytes() == want["ds"].tobytes() and ta.grad.cpu().numpy().tobytes() == want["da"].tobytes()


# ---- sed_crnn_backward_att -----------------------------------------------------------------------------------------------------------
WIDTHS = [dict(), dict(C=128, H=256)]
WIDTH_IDS = ["base", "wide"]
SEED = 424242


def _weights(B, T3, NC, seed=7):
    rs = np.random.RandomState(seed)
    return (torch.tensor(rs.standard_normal((B, T3, NC)), dtype=torch.float32), torch.tensor(rs.standard_normal((B, NC)), dtype=torch.float32),
            torch.tensor(rs.standard_normal((B, T3, NC)), dtype=torch.float32))


def _grads(loss_of, B, T, p, return_attention, **kw):
    """Parameter gradients of loss_of(strong, weak[, att]) on a fresh model (the same weights, input and dropout seed every time)."""
    model, _ = gu.make_model(0, dropout=p, **kw)
    model.train()
    x = synth.make_input(40, B, T).cuda()
    out = model(x, seed=gu.seed_tensor(SEED) if p > 0 else None, return_attention=return_attention)
    loss_of(*out).backward()
    torch.cuda.synchronize()
    return gu.grads_dict(model), [o.detach() for o in out]


@pytest.mark.parametrize("kw", WIDTHS, ids=WIDTH_IDS)
def test_null_attention_gradient_is_bit_identical_to_sed_crnn_backward(kw):
    """The loss does not use the attention: the node passes d_att = NULL."""
    B, T = 2, 64
    ws, ww, _ = _weights(B, T // 8, 10)
    loss = lambda s, w, att=None: (s * ws.cuda()).sum() + (w * ww.cuda()).sum()
    g0, out0 = _grads(loss, B, T, 0.5, False, **kw)
    g1, out1 = _grads(loss, B, T, 0.5, True, **kw)
    assert len(out1) == 3 and tuple(out1[2].shape) == (B, T // 8, 10)
    assert torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1])
    for n in g0:
        assert g0[n].numpy().tobytes() == g1[n].numpy().tobytes(), n


@pytest.mark.parametrize("kw", WIDTHS, ids=WIDTH_IDS)
def test_the_weak_gradient_routed_through_strong_and_attention_is_the_same_gradient(kw):
    """weak = sum_t strong att / den, den = sum_t att: backward(d_strong = 0, d_weak = dw) against
    backward_att(d_strong = dw att / den, d_att = dw (strong - weak) / den, d_weak = 0) - the same quantity in exact arithmetic,
    only heads-level rounding differs; _check_grads' bounds.  The attention is also the one last_attention() reads."""
    B, T = 2, 64
    _, dw, _ = _weights(B, T // 8, 10, seed=8)
    dw = dw.cuda()
    g0, _ = _grads(lambda s, w: (w * dw).sum(), B, T, 0.5, False, **kw)

    def routed(s, w, att):
        den = att.sum(1, keepdim=True)
        d_s = (dw[:, None, :] * att / den).detach()
        d_a = (dw[:, None, :] * (s - w[:, None, :]) / den).detach()
        return (s * d_s).sum() + (att * d_a).sum()

    g1, out = _grads(routed, B, T, 0.5, True, **kw)
    att = out[2].cpu().numpy()
    assert (att >= np.float32(1e-7)).all() and (att <= 1).all()
    worst = _check_grads(g1, g0)
    print(f"[backward_att vs backward, {kw or 'base'}] worst err/typ {worst:.3e}")


_ORACLE = {}


def _oracle_att(B, T, C, H):
    """float64 oracle of loss = sum ws strong + sum ww weak + sum wa att, att restated from the last GRU intermediate."""
    key = (B, T, C, H)
    if key not in _ORACLE:
        params = synth.make_params(0, n_layers_RNN=2, nclass=10, nb_filters=(C,) * 3, n_RNN_cell=H)
        po = {k: v.double().requires_grad_(True) for k, v in params.items()}
        x = synth.make_input(40, B, T).double()
        so, wo, inter = ref_cpu.crnn_forward(po, x, True, ref_cpu.new_bn_state([C] * 3, dtype=torch.float64), None, return_intermediates=True)
        att = torch.clamp(torch.softmax(torch.nn.functional.linear(inter["gru1"], po["dense_softmax.weight"], po["dense_softmax.bias"]), dim=-1),
                          min=1e-7, max=1)
        ws, ww, wa = (t.double() for t in _weights(B, T // 8, 10, seed=9))
        lo = (so * ws).sum() + (wo * ww).sum() + (att * wa).sum()
        go = dict(zip(po.keys(), torch.autograd.grad(lo, list(po.values()))))
        _ORACLE[key] = dict(go=go, att=att.detach(), so=so.detach(), wo=wo.detach())
    return _ORACLE[key]


@pytest.mark.parametrize("B,T", [(2, 64), (3, 22)])
@pytest.mark.parametrize("kw", WIDTHS, ids=WIDTH_IDS)
def test_backward_att_matches_the_float64_oracle(kw, B, T):
    ora = _oracle_att(B, T, kw.get("C", 64), kw.get("H", 64))
    ws, ww, wa = (t.cuda() for t in _weights(B, T // 8, 10, seed=9))
    g, out = _grads(lambda s, w, att: (s * ws).sum() + (w * ww).sum() + (att * wa).sum(), B, T, 0.0, True, **kw)
    assert float((out[2].cpu().double() - ora["att"]).abs().max()) < 2e-5
    assert float((out[0].cpu().double() - ora["so"]).abs().max()) < 2e-5 and float((out[1].cpu().double() - ora["wo"]).abs().max()) < 2e-5
    worst = _check_grads(g, {k: v.float() for k, v in ora["go"].items()})
    print(f"[backward_att vs float64 oracle, {kw or 'base'} ({B}, {T})] worst err/typ {worst:.3e}")


def test_backward_att_in_the_f16_mode_against_fp32():
    """mfma_dtype = "f16" against the fp32 result of the same call, at the per-layer-class bounds the f16 mode's
    sed_crnn_backward is held to (tests/test_gpu_generic.py: F16_GRAD_TOL)."""
    B, T = 2, 64
    ws, ww, wa = (t.cuda() for t in _weights(B, T // 8, 10, seed=10))
    loss = lambda s, w, att: (s * ws).sum() + (w * ww).sum() + (att * wa).sum()
    g32, _ = _grads(loss, B, T, 0.5, True)
    g16, _ = _grads(loss, B, T, 0.5, True, mfma_dtype="f16")
    cls = {}
    worst, name = _grad_errors(g16, g32, cls)
    print(f"[backward_att f16 vs f32] worst err/typ {worst:.3e} ({name}); per class " + " ".join(f"{k} {v:.2e}" for k, v in sorted(cls.items())))
    assert cls["cnn"] < F16_GRAD_TOL["cnn"] and cls["rnn"] < F16_GRAD_TOL["rnn64"] and cls["heads"] < F16_GRAD_TOL["heads"], cls


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _torch_pooled(strong, att, rec_win0, rec_frame0, T3, hop3):
    """The taper blend and the pooling restated in torch (whatever dtype the inputs have), differentiable."""
    rows = []
    for r in range(len(rec_win0) - 1):
        w0, nw, L3 = int(rec_win0[r]), int(rec_win0[r + 1] - rec_win0[r]), int(rec_frame0[r + 1] - rec_frame0[r])
        num = den = 0
        for u in range(L3):
            cover = [j for j in range(nw) if 0 <= u - j * hop3 < T3]
            wts = [min(u - j * hop3 + 1, T3 - (u - j * hop3)) for j in cover]
            if len(cover) == 1:
                p, a = strong[w0 + cover[0], u - cover[0] * hop3], att[w0 + cover[0], u - cover[0] * hop3]
            else:
                p = sum(w * strong[w0 + j, u - j * hop3] for j, w in zip(cover, wts)) / sum(wts)
                a = sum(w * att[w0 + j, u - j * hop3] for j, w in zip(cover, wts)) / sum(wts)
            num, den = num + p * a, den + a
        rows.append(num / den)
    return torch.stack(rows)


def test_one_backward_and_three_adam_steps_follow_the_float64_oracle():
    """Three recordings of 64, 100 and 160 frames at T = 64, hop 32 (1 + 2 + 4 windows, one batch), nclass 10, dropout 0: the
    parameter gradients of train_recording_tags' loss against float64 autograd through the oracle forward, the blend and the
    pooling (_check_grads' bounds), then three torch.optim.Adam(lr = 1e-3) steps: per-step losses within rel 2e-4 of the
    oracle trajectory (the bound of the 3-step trajectory test's meters)."""
    from dcase2019_task4_amd.inference import LongRecordingSet
    from dcase2019_task4_amd.train import recording_tags_loss, train_recording_tags
    FR, HOP, T3, hop3, NC = 64, 32, 8, 4, 10
    ls = LongRecordingSet.from_arrays(_recordings([64, 100, 160]), FR, hop_frames=HOP, scaler=_Scaler(64))
    assert list(np.diff(ls.rec_win0_host)) == [1, 2, 4] and ls.T3 == T3 and ls.hop3 == hop3
    tags = np.random.RandomState(12).uniform(size=(3, NC)).astype(np.float32)
    model, params = gu.make_model(0, dropout=0.0)
    model.train()
    runs, at, w0, f0 = ls.tag_batches(64)
    assert ls.tag_batches(64)[2] is w0                     # built once
    assert runs == [(0, 3)]
    loss, err = recording_tags_loss(ls, torch.from_numpy(tags).cuda(), model, runs[0], (0, at, w0, f0))
    loss.backward()
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    g = gu.grads_dict(model)
    # the oracle: float64 parameters, the same windows
    x = ls.eval_batch(0, 7).cpu().double()
    po = {k: v.double().requires_grad_(True) for k, v in params.items()}

    def oracle_loss():
        so, _, inter = ref_cpu.crnn_forward(po, x, True, ref_cpu.new_bn_state(dtype=torch.float64), None, return_intermediates=True)
        att = torch.clamp(torch.softmax(torch.nn.functional.linear(inter["gru1"], po["dense_softmax.weight"], po["dense_softmax.bias"]), dim=-1),
                          min=1e-7, max=1)
        weak = _torch_pooled(so, att, ls.rec_win0_host, ls.rec_frame0_host, T3, hop3)
        return torch.nn.functional.binary_cross_entropy(weak, torch.from_numpy(tags).double())

    lo = oracle_loss()
    go = dict(zip(po.keys(), torch.autograd.grad(lo, list(po.values()))))
    assert float(loss.detach()) == pytest.approx(float(lo.detach()), rel=1e-5)
    worst = _check_grads(g, {k: v.float() for k, v in go.items()})
    print(f"[recording tags, one backward] loss {float(loss.detach()):.6f} / {float(lo.detach()):.6f}; worst err/typ {worst:.3e}")
    # three steps
    model.zero_grad()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    got = [train_recording_tags(ls, tags, model, opt, epoch) for epoch in range(3)]
    opt_o = torch.optim.Adam(list(po.values()), lr=1e-3)
    want = []
    for _ in range(3):
        opt_o.zero_grad()
        lo = oracle_loss()
        lo.backward()
        opt_o.step()
        want.append(float(lo.detach()))
    dev = max(abs(a - b) / b for a, b in zip(got, want))
    print(f"[recording tags, three Adam steps] losses {got} / {want}; worst relative deviation {dev:.3e}")
    assert want[2] < want[0]
    assert dev <= 2e-4
    # with a teacher: the EMA of train() after the step, global_step = epoch * n_batches + i = 3 -> alpha = min(1 - 1 / 4, 0.999)
    teacher, _ = gu.make_model(1, dropout=0.0)
    teacher.flatten_parameters_()
    before = teacher._flat.clone()
    train_recording_tags(ls, tags, model, opt, 3, ema_model=teacher)
    torch.testing.assert_close(teacher._flat, 0.75 * before + 0.25 * model._flat, rtol=1e-6, atol=1e-7)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.crnn import CRNN
    from dcase2019_task4_amd.inference import LongRecordingSet
    from dcase2019_task4_amd.train import train_recording_tags
    stock = CRNN(**dict(gu.CRNN_KW, attention=False))
    assert not stock.hot_path
    with pytest.raises(_lib.SedError, match="hot path"):
        stock(torch.zeros(2, 1, 64, 64), return_attention=True)
    model, _ = gu.make_model(0, dropout=0.0)
    model.eval()
    x = synth.make_input(5, 2, 64).cuda()
    s, w, att = model(x, return_attention=True)
    with pytest.raises(_lib.SedError, match="eval-mode"):
        (s.sum() + att.sum()).backward()
    with torch.no_grad():
        s2, w2, att2 = model(x, return_attention=True)
    assert torch.equal(att2, model.last_attention()) and torch.equal(s, s2)
    with pytest.raises(_lib.SedError, match="input features"):
        model.train()
        model(x.clone().requires_grad_(True), return_attention=True)
    ls = LongRecordingSet.from_arrays(_recordings([64, 400]), 64, hop_frames=32, scaler=_Scaler(64))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="more than max_windows"):
        train_recording_tags(ls, np.zeros((2, 10), np.float32), model, opt, 0, max_windows=4)
    with pytest.raises(ValueError, match="tags"):
        train_recording_tags(ls, np.zeros((3, 10), np.float32), model, opt, 0)

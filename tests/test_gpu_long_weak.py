"""-m gpu tests of the recording-level weak tags of long recordings: sed_stitch_weak against the numpy statement
(tests/weak_np.py: the bitwise blend of tests/stitch_np.py, then math.fsum), its two consequences, error bits, bad arguments,
reproducibility and graph replay; sed_crnn_attention / CRNN.last_attention against the context of the forward; and
get_long_predictions(return_weak=True) / validate_long(weak_labels=...) end to end on a small model.  Every buffer a kernel
writes starts as NaN / sentinel bytes and carries a tail that must come back untouched."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

from tests import gpu_util as gu
from tests import weak_np
from tests.long_util import SENT, TAIL, _Scaler, _tables, _tile
from tests.test_gpu_long import FRAMES, LABELS, _recordings
from tests.test_gpu_parity import POST_TOL

pytestmark = pytest.mark.gpu

U32, U64 = 2.0 ** -24, 2.0 ** -53


def _ulps(got, want):
    """Distance in float32 steps between two arrays of finite non-negative floats."""
    g, w = np.ascontiguousarray(got, np.float32).view(np.int32).astype(np.int64), np.ascontiguousarray(want, np.float32).view(np.int32)
    return np.abs(g - w)


class WeakCall:
    """One sed_stitch_weak call on sentinel-filled outputs (NaN weak / sums with a tail of TAIL NaNs, 0xFF workspace with a
    tail, a second error word).  ``misalign``: "p" or "a" shifts that window tensor off 16-byte alignment."""

    def __init__(self, p, a, rec_win0, rec_frame0, hop3, weighting, misalign=None):
        from dcase2019_task4_amd import _lib
        self._lib, self.l = _lib, _lib.lib()
        p, a = np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(a, dtype=np.float32)
        self.n_win, self.T3, self.NC = p.shape
        self.n_rec, self.total = len(rec_win0) - 1, int(rec_frame0[-1])
        self.hop3, self.weighting = int(hop3), int(weighting)
        self._bufs = []
        for name, src in (("p", p), ("a", a)):
            off = 1 if misalign == name else 0
            buf = torch.empty(src.size + off, dtype=torch.float32, device="cuda")
            buf[off:].copy_(torch.from_numpy(src.reshape(-1)))
            assert (buf[off:].data_ptr() % 16 != 0) == bool(off)
            self._bufs.append(buf)
            setattr(self, name, buf[off:])
        self.rec_win0 = torch.from_numpy(np.asarray(rec_win0, dtype=np.int32)).cuda()
        self.rec_frame0 = torch.from_numpy(np.asarray(rec_frame0, dtype=np.int64)).cuda()
        n = self.n_rec * self.NC
        self.weak = torch.empty(n + TAIL, dtype=torch.float32, device="cuda")
        self.sums = torch.empty(2 * n + TAIL, dtype=torch.float64, device="cuda")
        self.err = torch.empty(2, dtype=torch.int32, device="cuda")
        self.ws_bytes = self.l.sed_stitch_weak_ws_bytes(self.total, self.n_rec, self.NC)
        assert self.ws_bytes > 0, self.l.sed_last_error()
        self.ws = torch.empty(self.ws_bytes + TAIL, dtype=torch.uint8, device="cuda")

    def fill(self):
        self.weak.fill_(float("nan"))
        self.sums.fill_(float("nan"))
        self.ws.fill_(0xFF)
        self.err.fill_(SENT)
        self.err[:1].zero_()

    def launch(self, **kw):
        ptr = self._lib.ptr
        a = dict(p=self.p, a=self.a, n_rec=self.n_rec, T3=self.T3, NC=self.NC, hop3=self.hop3, weighting=self.weighting,
                 weak=self.weak, sums=self.sums, ws=self.ws, ws_bytes=self.ws_bytes)
        a.update(kw)
        return self.l.sed_stitch_weak(ptr(a["p"]), ptr(a["a"]), ptr(self.rec_win0), ptr(self.rec_frame0), a["n_rec"], a["T3"],
                                      a["NC"], a["hop3"], a["weighting"], ptr(a["weak"]), ptr(a["sums"]), ptr(a["ws"]),
                                      a["ws_bytes"], ptr(self.err), self._lib.stream_ptr())

    def untouched(self):
        """Nothing was written: the outputs are still their sentinels and the error word is clear."""
        torch.cuda.synchronize()
        return bool(torch.isnan(self.weak).all() and torch.isnan(self.sums).all() and (self.ws == 0xFF).all()
                    and int(self.err[0].item()) == 0 and int(self.err[1].item()) == SENT)

    def get(self):
        torch.cuda.synchronize()
        n = self.n_rec * self.NC
        weak, sums = self.weak.cpu().numpy(), self.sums.cpu().numpy()
        assert np.isnan(weak[n:]).all() and np.isnan(sums[2 * n:]).all()
        assert int(self.err[1].item()) == SENT and (self.ws[-TAIL:] == 0xFF).all()
        return {"weak": weak[:n].reshape(self.n_rec, self.NC), "sums": sums[:2 * n].reshape(self.n_rec, self.NC, 2),
                "err": int(self.err[0].item())}

    def run(self):
        self.fill()
        assert self.launch() == 0, self.l.sed_last_error()
        return self.get()


def _inputs(rs, n_win, T3, NC):
    return rs.uniform(size=(n_win, T3, NC)).astype(np.float32), weak_np.attention(rs, n_win, T3, NC)


def _check(got, want_weak, want_sums, L3s, rows=None, what=""):
    """The issue's two bounds: sums within (L3 - 1) 2^-53 relative of the fsum values (any-order fp64 summation of
    non-negative terms), weak within one float32 step of the statement.  Prints how many tags are not bit-equal."""
    rows = range(len(L3s)) if rows is None else rows
    n_diff = 0
    for r in rows:
        bound = (L3s[r] - 1) * U64 * want_sums[r]
        assert (np.abs(got["sums"][r] - want_sums[r]) <= bound).all(), (what, r, got["sums"][r], want_sums[r])
        d = _ulps(got["weak"][r], want_weak[r])
        assert (d <= 1).all(), (what, r, got["weak"][r], want_weak[r])
        n_diff += int((d != 0).sum())
    print(f"{what}: {n_diff} of {len(list(rows)) * got['weak'].shape[1]} tags not bit-equal to the statement")


# ---- the kernel against the statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", [1, 3, 8])
@pytest.mark.parametrize("NC,misalign", [(1, None), (3, None), (10, None), (12, None), (12, "p"), (12, "a")])
def test_tags_and_sums_match_the_fsum_statement(NC, misalign, hop3, weighting):
    """Scalar path (NC = 1, 3, 10; NC = 12 with either input off 16-byte alignment) and 16-byte path (NC = 12); every length
    around the window and the tile as recordings of ONE call."""
    T3, t = 8, _tile()
    L3s = [1, 7, 8, 9, 8 + hop3, t - 1, t, t + 1, 2 * t + 5]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    rs = np.random.RandomState(1000 + 100 * NC + 10 * hop3 + weighting)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    assert (a == np.float32(1.0)).any() and (NC == 1 or (a == np.float32(1e-7)).any())
    got = WeakCall(p, a, rec_win0, rec_frame0, hop3, weighting, misalign=misalign).run()
    assert got["err"] == 0
    want_weak, want_sums = _reference(p, a, rec_win0, rec_frame0, hop3, weighting)
    _check(got, want_weak, want_sums, L3s, what=f"NC={NC} misalign={misalign} hop3={hop3} weighting={weighting}")
    if misalign is not None:                       # the summation order does not depend on the path: identical bytes
        aligned = WeakCall(p, a, rec_win0, rec_frame0, hop3, weighting).run()
        assert aligned["weak"].tobytes() == got["weak"].tobytes() and aligned["sums"].tobytes() == got["sums"].tobytes()


_REF = {}


def _reference(p, a, rec_win0, rec_frame0, hop3, weighting):
    """The statement, computed once per input (the misaligned cases share the aligned case's inputs)."""
    key = (p.tobytes(), a.tobytes(), tuple(rec_win0), tuple(rec_frame0), hop3, weighting)
    if key not in _REF:
        _REF.clear()
        _REF[key] = weak_np.pool(p, a, rec_win0, rec_frame0, hop3, weighting)
    return _REF[key]


# ---- the two consequences, on the kernel alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize("NC", [3, 12])
def test_single_window_recordings_pool_their_own_frames(NC):
    T3, hop3 = 8, 4
    L3s = [1, 2, 5, 7, 8, 8]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    assert list(np.diff(rec_win0)) == [1] * len(L3s)
    p, a = _inputs(np.random.RandomState(50 + NC), len(L3s), T3, NC)
    got = WeakCall(p, a, rec_win0, rec_frame0, hop3, 1).run()
    assert got["err"] == 0
    for r, L3 in enumerate(L3s):
        for c in range(NC):
            num = math.fsum(float(p[r, v, c]) * float(a[r, v, c]) for v in range(L3))
            den = math.fsum(float(a[r, v, c]) for v in range(L3))
            assert abs(got["sums"][r, c, 0] - num) <= (L3 - 1) * U64 * num and abs(got["sums"][r, c, 1] - den) <= (L3 - 1) * U64 * den
            assert _ulps(got["weak"][r, c], np.float32(num / den)) <= 1


@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("NC", [3, 12])
def test_disjoint_windows_give_the_den_weighted_mean_of_the_window_tags(NC, weighting):
    """hop3 == T3 and L3 a multiple of T3: weak[r] is the den-weighted mean of the tags the SAME kernel gives each window as a
    recording of its own (one window, 70 windows = more than one tile)."""
    T3 = 8
    n_w = [1, 3, 70]
    n = sum(n_w)
    p, a = _inputs(np.random.RandomState(60 + NC), n, T3, NC)
    whole = WeakCall(p, a, np.r_[0, np.cumsum(n_w)], np.r_[0, np.cumsum(n_w)] * T3, T3, weighting).run()
    each = WeakCall(p, a, np.arange(n + 1), np.arange(n + 1) * T3, T3, weighting).run()
    assert whole["err"] == 0 and each["err"] == 0
    w0 = 0
    for r, k in enumerate(n_w):
        den = each["sums"][w0:w0 + k, :, 1]
        mean = (den * each["weak"][w0:w0 + k].astype(np.float64)).sum(0) / den.sum(0)
        np.testing.assert_allclose(whole["weak"][r], mean, rtol=4 * U32, atol=0)
        w0 += k


# ---- error paths -------------------------------------------------------------------------------------------------------------------
def _one_recording(p, a, w0, nw, L3, hop3, weighting):
    return weak_np.pool(p[w0:w0 + nw], a[w0:w0 + nw], [0, nw], [0, L3], hop3, weighting)


def _check_bad_row(got, bad, valid, p, a, hop3):
    """Row `bad` is NaN in both outputs; every row of `valid` = {r: (w0, nw, L3)} is the statement on that recording alone."""
    assert np.isnan(got["weak"][bad]).all() and np.isnan(got["sums"][bad]).all()
    for r, (w0, nw, L3) in valid.items():
        want_weak, want_sums = _one_recording(p, a, w0, nw, L3, hop3, 0)
        _check({"weak": got["weak"][r:r + 1], "sums": got["sums"][r:r + 1]}, want_weak, want_sums, [L3], what=f"row {r}")


def test_too_few_windows_raise_bit_32_and_only_that_row_is_nan():
    """Recording 1 needs 4 windows and is given 2."""
    T3, NC = 8, 3
    p, a = _inputs(np.random.RandomState(70), 4, T3, NC)
    got = WeakCall(p, a, [0, 1, 3, 4], [0, 8, 38, 46], T3, 0).run()
    assert got["err"] == 32
    _check_bad_row(got, 1, {0: (0, 1, 8), 2: (3, 1, 8)}, p, a, T3)


@pytest.mark.parametrize("rec_win0,rec_frame0,valid", [
    ([0, 2, 1, 3], [0, 8, 16, 24], {0: (0, 2, 8), 2: (1, 2, 8)}),            # windows run backwards
    ([0, 3, 4, 6], [0, 20, 16, 30], {0: (0, 3, 20), 2: (4, 2, 14)}),        # frames run backwards
    ([0, 1, 9, 3], [0, 8, 16, 24], {0: (0, 1, 8)}),                          # windows beyond the table's own total
])
def test_malformed_tables_raise_bit_16_and_only_those_rows_are_nan(rec_win0, rec_frame0, valid):
    T3, NC = 8, 3
    p, a = _inputs(np.random.RandomState(71), 6, T3, NC)
    got = WeakCall(p, a, rec_win0, rec_frame0, T3, 0).run()
    assert got["err"] & 16 and not got["err"] & ~48
    bad = [r for r in range(3) if r not in valid]
    for r in bad:
        _check_bad_row(got, r, {}, p, a, T3)
    _check_bad_row(got, bad[0], valid, p, a, T3)


def test_more_tiles_than_the_workspace_holds_raise_bit_16():
    """A workspace sized for shorter tables (a whole number of slots, so the host accepts it): the recording whose tiles do
    not fit is refused, nothing is written beyond the workspace."""
    T3, NC, t = 8, 3, _tile()
    L3s = [8, 2 * t + 8]
    rec_win0, rec_frame0 = _tables(L3s, T3, T3)
    p, a = _inputs(np.random.RandomState(72), rec_win0[-1], T3, NC)
    call = WeakCall(p, a, rec_win0, rec_frame0, T3, 0)
    small = call.l.sed_stitch_weak_ws_bytes(16, 2, NC)
    call.ws_bytes, call.ws = small, torch.empty(small + TAIL, dtype=torch.uint8, device="cuda")
    got = call.run()
    assert got["err"] == 16
    _check_bad_row(got, 1, {0: (0, 1, 8)}, p, a, T3)


def test_bad_host_arguments_return_bad_arg_before_any_launch():
    T3, NC = 8, 3
    rec_win0, rec_frame0 = _tables([8, 20], T3, T3)
    p, a = _inputs(np.random.RandomState(73), rec_win0[-1], T3, NC)
    call = WeakCall(p, a, rec_win0, rec_frame0, T3, 0)
    call.fill()
    per_slot = NC * 16
    for kw in (dict(NC=17), dict(NC=0), dict(hop3=0), dict(hop3=9), dict(T3=0), dict(T3=4097, hop3=1), dict(weighting=2),
               dict(n_rec=0), dict(p=None), dict(a=None), dict(weak=None), dict(ws=None), dict(ws_bytes=call.ws_bytes + 8),
               dict(ws_bytes=2 * per_slot), dict(ws_bytes=0)):
        assert call.launch(**kw) == -1, kw                                       # SED_ERR_BAD_ARG
    assert call.untouched()
    l = call.l
    assert l.sed_stitch_weak_ws_bytes(1 << 28, 1, 10) == 0 and l.sed_stitch_weak_ws_bytes(100, 1, 17) == 0
    assert l.sed_stitch_weak_ws_bytes(0, 1, 10) == 0 and l.sed_stitch_weak_ws_bytes(100, 0, 10) == 0
    assert l.sed_stitch_weak_ws_bytes(2 * _tile() + 5, 3, 10) == (2 + 3 + 1) * 10 * 16
    assert call.launch(sums=None) == 0                                            # sums is optional
    got = call.get()
    assert got["err"] == 0 and np.isnan(got["sums"]).all() and not np.isnan(got["weak"]).any()


def test_two_calls_and_a_graph_replay_give_identical_bytes():
    T3, NC, hop3 = 8, 10, 3
    L3s = [3 * _tile() + 9, 5, 40]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    p, a = _inputs(np.random.RandomState(74), rec_win0[-1], T3, NC)
    call = WeakCall(p, a, rec_win0, rec_frame0, hop3, 1)
    first = call.run()
    second = call.run()
    assert first["err"] == 0 and not np.isnan(first["weak"]).any()
    graph = torch.cuda.CUDAGraph()
    call.fill()
    with torch.cuda.graph(graph):
        assert call.launch() == 0
    call.fill()
    graph.replay()
    third = call.get()
    for other in (second, third):
        assert other["err"] == 0
        assert first["weak"].tobytes() == other["weak"].tobytes() and first["sums"].tobytes() == other["sums"].tobytes()


# ---- the attention of a forward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("kw", [dict(), dict(C=128, H=256, mfma_dtype="bf16")], ids=["f32", "wide-bf16"])
def test_attention_is_the_clamped_softmax_of_the_saved_logits(kw, train):
    from oracle import synth
    model, _ = gu.make_model(0, dropout=0.5, **kw)
    model.train(train)
    B, T = 3, 64
    x = synth.make_input(5, B, T).cuda()
    with torch.no_grad():
        _, weak = model(x, seed=gu.seed_tensor(11)) if train else model(x)
    att = model.last_attention()
    assert tuple(att.shape) == (B, T // 8, 10) and att.dtype == torch.float32
    att = att.cpu().numpy()
    logits = model.ctx_view("logits_s").cpu().numpy().reshape(B, T // 8, 10).astype(np.float64)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    want = np.clip(e / e.sum(-1, keepdims=True), 1e-7, 1.0)
    err = np.abs(att - want).max()
    print(f"attention vs float64 clamp(softmax): max abs error {err:.3e}")
    assert err <= POST_TOL
    assert (att >= np.float32(1e-7)).all() and (att <= 1.0).all()
    den = model.ctx_view("den").cpu().numpy().reshape(B, 10).astype(np.float64)
    T3 = T // 8
    mass = np.array([[math.fsum(float(v) for v in att[b, :, c]) for c in range(10)] for b in range(B)])
    rel = np.abs(mass - den) / den
    print(f"fsum of the attention vs the forward's den: max relative difference {rel.max():.3e}")
    assert (rel <= (T3 - 1) * U32).all()


def test_last_attention_refuses_what_it_cannot_read():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.crnn import CRNN
    from oracle import synth
    model, _ = gu.make_model(0)
    model.eval()
    with pytest.raises(_lib.SedError, match="no forward"):
        model.last_attention()
    with torch.no_grad():
        model(synth.make_input(5, 2, 64).cuda())
    model.last_attention()
    model.float().cpu().cuda()                         # parameters move: the flat buffer is rebuilt by the next forward
    model.flatten_parameters_()
    with pytest.raises(_lib.SedError, match="re-laid-out"):
        model.last_attention()
    stock = CRNN(**dict(gu.CRNN_KW, attention=False))
    assert not stock.hot_path
    with pytest.raises(_lib.SedError, match="hot path"):
        stock.last_attention()


def test_attention_bad_arguments():
    import ctypes as C
    from dcase2019_task4_amd import _lib
    l = _lib.lib()
    d = _lib.make_dims(2, 64)
    n = l.sed_crnn_ctx_bytes(C.byref(d))
    ctx = torch.zeros(n, dtype=torch.uint8, device="cuda")
    att = torch.full((2 * 8 * 10 + TAIL,), float("nan"), device="cuda")
    go = lambda dims=d, c=ctx, nb=n, out=att: l.sed_crnn_attention(C.byref(dims), _lib.ptr(c), nb, _lib.ptr(out), _lib.stream_ptr())
    assert go(dims=_lib.make_dims(2, 64, F=128)) == -1 and go(dims=_lib.make_dims(2, 64, nclass=17)) == -1
    assert go(nb=n - 1) == -1 and go(c=None) == -1 and go(out=None) == -1
    torch.cuda.synchronize()
    assert torch.isnan(att).all()
    assert go() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(att[:160]).any() and torch.isnan(att[160:]).all()


# ---- end to end, small model ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e():
    from dcase2019_task4_amd.inference import LongRecordingSet, get_long_predictions, long_window_posteriors
    model, _ = gu.make_model(0)
    model.eval()
    ls = LongRecordingSet.from_arrays(_recordings([40, 64, 300]), FRAMES, scaler=_Scaler(64), filenames=["a.wav", "b.wav", "c.wav"])
    df, _, win_strong, weak = get_long_predictions(model, ls, LABELS, batch_size=4, return_posteriors=True, return_weak=True)
    win_strong2, win_att = long_window_posteriors(model, ls, 10, batch_size=4, want_attention=True)
    assert win_strong2.cpu().numpy().tobytes() == win_strong.cpu().numpy().tobytes()
    return dict(model=model, ls=ls, df=df, weak=weak, win_strong=win_strong, win_att=win_att, get=get_long_predictions)


@pytest.mark.parametrize("weighting", ["taper", "uniform"])
def test_e2e_tags_equal_the_statement_on_the_windows(e2e, weighting):
    ls = e2e["ls"]
    out = e2e["get"](e2e["model"], ls, LABELS, batch_size=4, weighting=weighting, return_weak=True)
    assert isinstance(out, tuple) and len(out) == 2
    weak = out[1]
    assert weak.is_cuda and tuple(weak.shape) == (3, 10) and weak.dtype == torch.float32
    want, _ = weak_np.pool(e2e["win_strong"].cpu().numpy(), e2e["win_att"].cpu().numpy(), ls.rec_win0_host, ls.rec_frame0_host,
                           ls.hop3, {"uniform": 0, "taper": 1}[weighting])
    d = _ulps(weak.cpu().numpy(), want)
    print(f"{weighting}: {int((d != 0).sum())} of 30 tags not bit-equal to the statement")
    assert (d <= 1).all()
    if weighting == "taper":
        assert weak.cpu().numpy().tobytes() == e2e["weak"].cpu().numpy().tobytes()


def test_e2e_events_do_not_depend_on_return_weak(e2e):
    thr = float(np.median(e2e["win_strong"].cpu().numpy()))
    plain = e2e["get"](e2e["model"], e2e["ls"], LABELS, batch_size=4, threshold=thr)
    with_weak, _ = e2e["get"](e2e["model"], e2e["ls"], LABELS, batch_size=4, threshold=thr, return_weak=True)
    assert len(plain) > 0
    pd.testing.assert_frame_equal(plain, with_weak)
    assert plain.to_csv(sep="\t").encode() == with_weak.to_csv(sep="\t").encode()


def test_e2e_single_window_recordings_reproduce_the_clip_level_tag(e2e):
    """A recording that is exactly ONE FULL window (b.wav, and five recordings of `FRAMES` frames): its tag is the model's
    clip-level weak of that window up to the heads kernel's fp32 sums - within (2 T3 + 1) 2^-24 relative.  a.wav (5 label
    frames in a padded window of 8) is a single window too, but the clip-level tag pools the three padded frames, which by
    definition never enter the recording's sums: its figure is printed, and it is pinned by the statement above instead."""
    from dcase2019_task4_amd.inference import LongRecordingSet
    model, ls, T3 = e2e["model"], e2e["ls"], 8
    bound = (2 * T3 + 1) * U32
    with torch.no_grad():
        _, clip_weak = model(ls.eval_batch(0, 4))                                 # the first batch of the fixture's pass
    clip_weak, weak = clip_weak.cpu().numpy().astype(np.float64), e2e["weak"].cpu().numpy().astype(np.float64)
    rel = np.abs(weak[:2] - clip_weak[:2]) / clip_weak[:2]
    print(f"a.wav (L3 = 5 of 8): max relative difference {rel[0].max():.3e}; b.wav (L3 = 8): {rel[1].max():.3e}; bound {bound:.3e}")
    assert (rel[1] <= bound).all()
    clips = LongRecordingSet.from_arrays(_recordings([FRAMES] * 5, seed=33), FRAMES, scaler=_Scaler(64),
                                         filenames=[f"clip_{i}.wav" for i in range(5)])
    _, tags = e2e["get"](model, clips, LABELS, batch_size=5, return_weak=True)
    with torch.no_grad():
        _, clip_weak = model(clips.eval_batch(0, 5))
    clip_weak, tags = clip_weak.cpu().numpy().astype(np.float64), tags.cpu().numpy().astype(np.float64)
    rel = np.abs(tags - clip_weak) / clip_weak
    print(f"five full single-window recordings: max relative difference {rel.max():.3e}")
    assert (rel <= bound).all()


def test_e2e_validate_long_scores_the_tags(e2e):
    from dcase2019_task4_amd import metrics as M
    from tests.long_util import _ref_events
    model, ls = e2e["model"], e2e["ls"]
    weak = e2e["weak"].cpu().numpy()
    rs = np.random.RandomState(5)
    cols = [[[(0.1, 0.4)] if rs.uniform() < 0.5 else [] for _ in range(10)] for _ in range(3)]
    ref = _ref_events(cols)
    ref.labels = LABELS
    want_labels = np.array([[len(c) > 0 for c in rec] for rec in cols])
    np.testing.assert_array_equal(ref.weak_labels(), want_labels)
    med = np.median(weak, axis=0).astype(np.float32)                             # per-class thresholds that split the tags
    thresholds = [0.5, med, float(np.median(weak))]
    today = M.validate_long(model, ls, ref, thresholds, [3], batch_size=4)
    res, scored = M.validate_long(model, ls, ref, thresholds, [3], batch_size=4, weak_labels="from_ref")
    assert len(res) == len(today) == 3
    for (e0, s0), (e1, s1) in zip(today, res):
        assert e0.class_wise == e1.class_wise and s0.class_wise == s1.class_wise and s0.Ntn == s1.Ntn
    assert scored["counts"].shape == (3, 10, 4) and scored["counts"].dtype == np.int64
    for k, t in enumerate(thresholds):
        pred = weak > np.broadcast_to(np.asarray(t, np.float32), (10,))[None, :]
        want = np.stack([(pred & want_labels).sum(0), (pred & ~want_labels).sum(0), (~pred & want_labels).sum(0),
                         (~pred & ~want_labels).sum(0)], axis=1)
        np.testing.assert_array_equal(scored["counts"][k], want)
    np.testing.assert_array_equal(scored["f_measure"], M.f_measure_from_counts(scored["counts"]))
    assert scored["counts"][1, :, :2].sum() > 0                                   # the per-class thresholds predict some tags
    # an explicit label array and thresholds of their own
    _, other = M.validate_long(model, ls, ref, [0.5], [3], batch_size=4, weak_labels=want_labels.astype(np.uint8), weak_thresholds=[med])
    np.testing.assert_array_equal(other["counts"][0], scored["counts"][1])

"""-m gpu tests of training on span-level tags: sed_stitch_span_tags_backward against the float64 statement
(tests/span_tags_bwd_np.py) on the GPU forward's sums, bit-identity with sed_stitch_weak_backward at one span per recording,
position independence, error bits, bad arguments, reproducibility and graph replay; inference.pooled_span_tags against the direct
call; train.span_tags_loss with unknown (NaN) targets; and one epoch of train.train_span_tags against train_recording_tags.
Every buffer a kernel writes starts as 0xFF bytes and carries a tail that must come back untouched."""
import copy

import numpy as np
import pytest
import torch

from tests import gpu_util as gu
from tests import span_tags_bwd_np, span_tags_np, stitch_np, weak_np
from tests.long_util import SENT, TAIL, _Scaler, _tables, _tile
from tests.test_gpu_long import _recordings
from tests.test_gpu_long_weak_bwd import BwdCall, _step32
from tests.test_gpu_span_tags import SpanCall

pytestmark = pytest.mark.gpu


def _fwd(p, a, rec_win0, rec_frame0, hop3, weighting, span3):
    """The GPU forward's (num, den) sums [total_spans, NC, 2] and its error word."""
    out = SpanCall(p, a, rec_win0, rec_frame0, hop3, weighting, span3).run()
    return out["sums"], out["err"]


class SpanBwdCall:
    """One sed_stitch_span_tags_backward call on the ``sums`` handed in (the GPU forward's): both outputs start as 0xFF bytes
    with a tail of TAIL floats, a second error word.  ``misalign``: one of "p", "a", "ds", "da" shifts that tensor off 16 bytes;
    ``rec_span0`` / ``total_spans``: the table and the total given to the call (default: the right ones)."""

    def __init__(self, p, a, rec_win0, rec_frame0, hop3, weighting, span3, g, sums, misalign=None, rec_span0=None, total_spans=None):
        from dcase2019_task4_amd import _lib
        self._lib, self.l = _lib, _lib.lib()
        p, a = np.ascontiguousarray(p, dtype=np.float32), np.ascontiguousarray(a, dtype=np.float32)
        self.n_win, self.T3, self.NC = p.shape
        self.n_rec, self.hop3, self.weighting, self.span3 = len(rec_win0) - 1, int(hop3), int(weighting), int(span3)
        self.n = p.size
        self.span0_host = span_tags_np.span_table(np.diff(np.asarray(rec_frame0, np.int64)), self.span3) if rec_span0 is None \
            else np.asarray(rec_span0, np.int64)
        self.total_spans = int(self.span0_host[-1]) if total_spans is None else int(total_spans)
        self.sums = torch.from_numpy(np.ascontiguousarray(sums, dtype=np.float64)).cuda()
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
        self.rec_span0 = torch.from_numpy(self.span0_host).cuda()
        self.err = torch.empty(2, dtype=torch.int32, device="cuda")

    def fill(self):
        for name in ("ds", "da"):
            getattr(self, name).view(torch.int32).fill_(-1)          # 0xFF bytes
        self.err.fill_(SENT)
        self.err[:1].zero_()

    def launch(self, **kw):
        ptr = self._lib.ptr
        k = dict(p=self.p, a=self.a, n_rec=self.n_rec, T3=self.T3, NC=self.NC, hop3=self.hop3, weighting=self.weighting,
                 span3=self.span3, total_spans=self.total_spans, sums=self.sums, g=self.g, ds=self.ds, da=self.da, err=self.err,
                 w0=self.rec_win0, f0=self.rec_frame0, s0=self.rec_span0)
        k.update(kw)
        return self.l.sed_stitch_span_tags_backward(ptr(k["p"]), ptr(k["a"]), ptr(k["w0"]), ptr(k["f0"]), ptr(k["s0"]),
                                                    k["total_spans"], k["n_rec"], k["T3"], k["NC"], k["hop3"], k["weighting"],
                                                    k["span3"], ptr(k["sums"]), ptr(k["g"]), ptr(k["ds"]), ptr(k["da"]),
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


def _g(rs, n_rows, NC):
    """Span gradients with zero entries and, from three rows on, whole zero rows."""
    g = rs.standard_normal((n_rows, NC)).astype(np.float32)
    g[rs.uniform(size=g.shape) < 0.15] = 0.0
    g[0, 0] = 0.0
    if n_rows >= 3:
        g[1::5] = 0.0
    return g


def _check(got, want, what):
    """Every element within one float32 step of the statement (the same fp64 operations in the same order; the step is for a
    last-bit difference in an fp64 division)."""
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


def _reference(seed, span3, p, a, rec_win0, rec_frame0, hop3, weighting, g):
    """The forward's sums and the statement on them, computed once per (inputs, span3): the misaligned cases share the aligned
    case's.  The two blends are shared by all the span lengths of one input."""
    if _REF.get("seed") != seed:
        _REF.clear()
        _REF["seed"] = seed
        _REF["blends"] = (stitch_np.blend(p, rec_win0, rec_frame0, hop3, weighting), stitch_np.blend(a, rec_win0, rec_frame0, hop3, weighting))
    if span3 not in _REF:
        sums, err = _fwd(p, a, rec_win0, rec_frame0, hop3, weighting, span3)
        assert err == 0
        _REF[span3] = (sums, span_tags_bwd_np.backward(p, a, rec_win0, rec_frame0, hop3, weighting, span3, g, sums=sums,
                                                       blends=_REF["blends"]))
    return _REF[span3]


@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", [1, 3, 8])
@pytest.mark.parametrize("NC,misalign", [(1, None), (3, None), (10, None), (12, None), (12, "p"), (12, "a"), (12, "ds"), (12, "da")])
def test_gradients_match_the_float64_statement(NC, misalign, hop3, weighting):
    """Scalar path (NC = 1, 3, 10; NC = 12 with any of the four window tensors off 16 bytes) and 16-byte path (NC = 12); span
    lengths of one frame, with a short last span, of one window and around the tile.  The full cross product with the span
    lengths for aligned NC = 3 and 12; the other cases take span3 = 3 and tile + 1."""
    T3, t = 8, _tile()
    L3s = [1, 5, 8, 9, 23, 2 * t + 5]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    seed = 3000 + 100 * NC + 10 * hop3 + weighting
    rs = np.random.RandomState(seed)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    span3s = [1, 3, 8, t - 1, t, t + 1] if NC in (3, 12) and misalign is None else [3, t + 1]
    for span3 in span3s:
        total_spans = int(span_tags_np.span_table(L3s, span3)[-1])
        g = _g(np.random.RandomState(seed + span3), total_spans, NC)
        assert (g == 0).any() and (g == 0).all(axis=1).any() and (g != 0).any()
        sums, want = _reference(seed, span3, p, a, rec_win0, rec_frame0, hop3, weighting, g)
        got = SpanBwdCall(p, a, rec_win0, rec_frame0, hop3, weighting, span3, g, sums, misalign=misalign).run()
        assert got["err"] == 0
        _check(got, want, f"NC={NC} misalign={misalign} hop3={hop3} weighting={weighting} span3={span3}")
        assert _tails_are_plus_zero(got, rec_win0, rec_frame0, T3, hop3) > 0
        if misalign is not None:                       # the 16-byte path and the scalar path: identical bytes
            aligned = SpanBwdCall(p, a, rec_win0, rec_frame0, hop3, weighting, span3, g, sums).run()
            assert aligned["ds"].tobytes() == got["ds"].tobytes() and aligned["da"].tobytes() == got["da"].tobytes()


@pytest.mark.parametrize("NC,hop3", [(3, 3), (12, 1), (12, 8)])
def test_one_span_per_recording_is_sed_stitch_weak_backward_bit_for_bit(NC, hop3):
    T3, t = 8, _tile()
    L3s = [1, 7, 8, 9, t + 1, 2 * t + 5]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    rs = np.random.RandomState(50 + NC + hop3)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    g = _g(rs, len(L3s), NC)
    weak = BwdCall(p, a, rec_win0, rec_frame0, hop3, 1, g)
    want = weak.run()
    assert want["err"] == 0 and want["ds"].any() and want["da"].any()
    for span3 in (max(L3s), max(L3s) + 7, 2 ** 31 - 1):
        call = SpanBwdCall(p, a, rec_win0, rec_frame0, hop3, 1, span3, g, weak.sums_host)
        assert call.span0_host.tolist() == list(range(len(L3s) + 1))
        got = call.run()
        assert got["err"] == 0
        assert got["ds"].tobytes() == want["ds"].tobytes() and got["da"].tobytes() == want["da"].tobytes()


# ---- position independence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NC", [3, 12])
def test_equal_recordings_with_equal_span_gradients_give_equal_bytes(NC):
    """Two recordings with the same windows - the second starts off the tile grid of the first - and the same span gradients."""
    T3, hop3, span3 = 8, 3, 8
    L = _tile() + 37
    rec_win0, rec_frame0 = _tables([L, 9, L], T3, hop3)
    rs = np.random.RandomState(60 + NC)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    nw = int(rec_win0[1])
    p[rec_win0[2]:], a[rec_win0[2]:] = p[:nw], a[:nw]
    span0 = span_tags_np.span_table([L, 9, L], span3)
    g = _g(rs, int(span0[-1]), NC)
    g[span0[2]:] = g[:span0[1]]
    sums, err = _fwd(p, a, rec_win0, rec_frame0, hop3, 1, span3)
    assert err == 0 and sums[span0[2]:].tobytes() == sums[:span0[1]].tobytes()
    got = SpanBwdCall(p, a, rec_win0, rec_frame0, hop3, 1, span3, g, sums).run()
    assert got["err"] == 0 and got["ds"][:nw].any() and got["da"][:nw].any()
    for name in ("ds", "da"):
        assert got[name][:nw].tobytes() == got[name][rec_win0[2]:].tobytes(), name


@pytest.mark.parametrize("NC", [3, 12])
def test_equal_spans_of_one_recording_give_equal_bytes(NC):
    """hop3 = T3 and windows repeating with a period of three: every span of 3 * T3 frames holds the same frames, wherever it
    lies relative to the tiles (the tile length is no multiple of 24), and every span gets the same gradient row."""
    T3, span3 = 8, 24
    n_sp = 2 * _tile() // span3 + 3
    assert _tile() % span3 != 0
    rec_win0, rec_frame0 = _tables([n_sp * span3], T3, T3)
    rs = np.random.RandomState(70 + NC)
    p3, a3 = _inputs(rs, 3, T3, NC)
    p, a = np.tile(p3, (n_sp, 1, 1)), np.tile(a3, (n_sp, 1, 1))
    g = np.tile(rs.standard_normal((1, NC)).astype(np.float32), (n_sp, 1))
    sums, err = _fwd(p, a, rec_win0, rec_frame0, T3, 0, span3)
    assert err == 0 and all(sums[s].tobytes() == sums[0].tobytes() for s in range(n_sp))
    got = SpanBwdCall(p, a, rec_win0, rec_frame0, T3, 0, span3, g, sums).run()
    assert got["err"] == 0 and got["ds"][:3].all() and got["da"][:3].any()
    for name in ("ds", "da"):
        for s in range(1, n_sp):
            assert got[name][3 * s:3 * s + 3].tobytes() == got[name][:3].tobytes(), (name, s)


# ---- error paths -------------------------------------------------------------------------------------------------------------------
def _bad_tables_case(rec_win0, rec_frame0, rec_span0, total_spans, valid, n_win, span3, seed):
    """One call on tables of which only the recordings of ``valid`` = {r: (w0, nw, L3)} are well-formed: their sums come from a
    forward of that recording alone and sit at the rows the given span table names.  Returns (call, got)."""
    T3, NC = 8, 3
    rs = np.random.RandomState(seed)
    p, a = _inputs(rs, 6, T3, NC)
    rows = max(int(total_spans), int(max(rec_span0))) + 4
    g = _g(rs, rows, NC)
    sums = np.full((rows, NC, 2), np.nan)
    for r, (w0, nw, L3) in valid.items():
        s_r, err = _fwd(p[w0:w0 + nw], a[w0:w0 + nw], [0, nw], [0, L3], T3, 0, span3)
        assert err == 0
        sums[rec_span0[r]:rec_span0[r] + len(s_r)] = s_r
    call = SpanBwdCall(p, a, rec_win0, rec_frame0, T3, 0, span3, g, sums, rec_span0=rec_span0, total_spans=total_spans)
    got = call.run()
    zero = np.zeros(p.shape[1:], np.float32).tobytes()
    owned = set()
    for r, (w0, nw, L3) in valid.items():
        n_sp = -(-L3 // span3)
        want = span_tags_bwd_np.backward(p[w0:w0 + nw], a[w0:w0 + nw], [0, nw], [0, L3], T3, 0, span3,
                                         g[rec_span0[r]:rec_span0[r] + n_sp], sums=sums[rec_span0[r]:rec_span0[r] + n_sp])
        _check({"ds": got["ds"][w0:w0 + nw], "da": got["da"][w0:w0 + nw]}, want, f"recording {r}")
        assert got["ds"][w0:w0 + nw].any()
        owned.update(range(w0, w0 + nw))
    for w in range(n_win):
        if w not in owned:
            assert got["ds"][w].tobytes() == zero and got["da"][w].tobytes() == zero, w
    # beyond rec_win0[n_rec] nothing is written: the call owns [0, n_win) only
    assert (call.ds[n_win * T3 * NC:].view(torch.int32) == -1).all() and (call.da[n_win * T3 * NC:].view(torch.int32) == -1).all()
    return call, got


def test_too_few_windows_raise_bit_32_and_those_windows_are_zero():
    """Recording 1 needs 4 windows and is given 2 (hop3 = T3 = 8, span3 = 8)."""
    _, got = _bad_tables_case([0, 1, 3, 4], [0, 8, 38, 46], [0, 1, 5, 6], 6, {0: (0, 1, 8), 2: (3, 1, 8)}, 4, 8, 190)
    assert got["err"] == 32


@pytest.mark.parametrize("rec_win0,rec_frame0,rec_span0,total_spans,valid,n_win", [
    ([0, 3, 4, 6], [0, 20, 16, 30], [0, 3, 3, 5], 5, {0: (0, 3, 20), 2: (4, 2, 14)}, 6),      # frames run backwards
    ([0, 1, 9, 3], [0, 8, 16, 24], [0, 1, 2, 3], 3, {0: (0, 1, 8)}, 3),                       # windows beyond the table's total
    ([0, 3, 4, 6], [0, 20, 28, 42], [0, 3, 5, 7], 7, {0: (0, 3, 20), 2: (4, 2, 14)}, 6),      # one span too many for recording 1
    ([0, 3, 4, 6], [0, 20, 28, 42], [0, 2, 3, 5], 5, {1: (3, 1, 8), 2: (4, 2, 14)}, 6),       # one span too few for recording 0
    ([0, 3, 4, 6], [0, 20, 28, 42], [0, 3, 4, 6], 5, {0: (0, 3, 20), 1: (3, 1, 8)}, 6),       # rec_span0 beyond total_spans
    ([0, 3, 4, 6], [0, 20, 28, 42], [4, 3, 4, 6], 6, {1: (3, 1, 8), 2: (4, 2, 14)}, 6),       # spans run backwards
    ([0, 3, 4, 6], [0, 20, 28, 42], [-3, 0, 1, 3], 3, {1: (3, 1, 8), 2: (4, 2, 14)}, 6),      # a negative span offset
])
def test_malformed_tables_raise_bit_16_and_those_windows_are_zero(rec_win0, rec_frame0, rec_span0, total_spans, valid, n_win):
    _, got = _bad_tables_case(rec_win0, rec_frame0, rec_span0, total_spans, valid, n_win, 8, 191)
    assert got["err"] & 16 and not got["err"] & ~48


def _small_call(seed=193):
    T3, NC, span3 = 8, 3, 8
    rec_win0, rec_frame0 = _tables([8, 20], T3, T3)
    rs = np.random.RandomState(seed)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    sums, err = _fwd(p, a, rec_win0, rec_frame0, T3, 0, span3)
    assert err == 0
    return SpanBwdCall(p, a, rec_win0, rec_frame0, T3, 0, span3, _g(rs, len(sums), NC), sums)


def test_bad_host_arguments_return_bad_arg_before_any_launch():
    call = _small_call()
    assert call.total_spans == 4
    call.fill()
    odd_sums = torch.zeros(2 * call.sums.numel() + 2, dtype=torch.float32, device="cuda")[1:]     # 4 bytes off 8-byte alignment
    assert odd_sums.data_ptr() % 8 == 4
    for kw in (dict(NC=17), dict(NC=0), dict(hop3=0), dict(hop3=9), dict(T3=0), dict(T3=4097, hop3=1), dict(weighting=2),
               dict(n_rec=0), dict(span3=0), dict(span3=-8), dict(total_spans=1), dict(total_spans=2 ** 31 // 3 + 1), dict(total_spans=2 ** 62),
               dict(sums=odd_sums), dict(p=None), dict(a=None), dict(w0=None), dict(f0=None), dict(s0=None), dict(sums=None),
               dict(g=None), dict(ds=None), dict(da=None), dict(err=None)):
        assert call.launch(**kw) == -1, kw                                       # SED_ERR_BAD_ARG
    assert call.untouched()
    assert call.launch() == 0
    assert call.get()["err"] == 0


def test_two_calls_and_a_graph_replay_give_identical_bytes():
    T3, NC, hop3, span3 = 8, 10, 3, 31
    L3s = [3 * _tile() + 9, 5, 40]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    rs = np.random.RandomState(194)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    sums, err = _fwd(p, a, rec_win0, rec_frame0, hop3, 1, span3)
    assert err == 0
    call = SpanBwdCall(p, a, rec_win0, rec_frame0, hop3, 1, span3, _g(rs, len(sums), NC), sums)
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
@pytest.mark.parametrize("NC,span3", [(10, 5), (12, 600)])
def test_pooled_span_tags_backward_gives_the_bytes_of_the_direct_call(NC, span3):
    from dcase2019_task4_amd.inference import pooled_span_tags, stitch_span_tags
    T3, hop3 = 8, 3
    L3s = [_tile() + 9, 5, 40]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    rs = np.random.RandomState(195 + NC)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    tp, ta = torch.from_numpy(p).cuda().requires_grad_(True), torch.from_numpy(a).cuda().requires_grad_(True)
    w0, f0 = torch.from_numpy(rec_win0).cuda(), torch.from_numpy(rec_frame0).cuda()
    out = pooled_span_tags(tp, ta, w0, f0, int(rec_frame0[-1]), hop3, span3, n_win=int(rec_win0[-1]), rec_frame0_host=rec_frame0)
    plain = stitch_span_tags(tp.detach(), ta.detach(), w0, f0, int(rec_frame0[-1]), hop3, span3, want_sums=True,
                             rec_frame0_host=rec_frame0)
    assert out["total_spans"] == plain["total_spans"] and out["span3"] == plain["span3"] == min(span3, max(L3s))
    assert out["rec_span0_host"].tolist() == plain["rec_span0_host"].tolist() and torch.equal(out["rec_span0"], plain["rec_span0"])
    assert out["tags"].requires_grad and torch.equal(out["tags"].detach(), plain["tags"])
    g = _g(rs, out["total_spans"], NC)
    out["tags"].backward(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    assert int(out["err"].item()) == 0
    want = SpanBwdCall(p, a, rec_win0, rec_frame0, hop3, 1, out["span3"], g, plain["sums"].cpu().numpy()).run()
    assert want["err"] == 0 and want["ds"].any() and want["da"].any()
    assert tp.grad.cpu().numpy().tobytes() == want["ds"].tobytes() and ta.grad.cpu().numpy().tobytes() == want["da"].tobytes()
    # a span table the caller prepared: the same node, nothing copied; one that is not these recordings' is refused
    tp.grad = ta.grad = None
    again = pooled_span_tags(tp, ta, w0, f0, int(rec_frame0[-1]), hop3, span3, n_win=int(rec_win0[-1]), rec_frame0_host=rec_frame0,
                             span_tables=(out["rec_span0_host"], out["rec_span0"]))
    again["tags"].backward(torch.from_numpy(g).cuda())
    assert again["rec_span0"] is out["rec_span0"] and tp.grad.cpu().numpy().tobytes() == want["ds"].tobytes()
    with pytest.raises(ValueError, match="span_tables"):
        pooled_span_tags(tp, ta, w0, f0, int(rec_frame0[-1]), hop3, span3, rec_frame0_host=rec_frame0,
                         span_tables=(out["rec_span0_host"] + 1, out["rec_span0"]))
    with pytest.raises(ValueError, match="int32"):
        pooled_span_tags(tp, ta, w0.long(), f0, int(rec_frame0[-1]), hop3, span3, rec_frame0_host=rec_frame0)
    with pytest.raises(ValueError, match="int32"):
        pooled_span_tags(tp, ta, w0, f0.cpu(), int(rec_frame0[-1]), hop3, span3, rec_frame0_host=rec_frame0)


# ---- the loss and the epoch ------------------------------------------------------------------------------------------------------
FR, HOP, NCLS = 64, 32, 10


def _small_set():
    from dcase2019_task4_amd.inference import LongRecordingSet
    ls = LongRecordingSet.from_arrays(_recordings([64, 96, 128]), FR, hop_frames=HOP, scaler=_Scaler(64))
    assert list(np.diff(ls.rec_win0_host)) == [1, 2, 3] and ls.T3 == 8 and ls.hop3 == 4
    assert list(np.diff(ls.rec_frame0_host)) == [8, 12, 16]
    return ls


class _Heads:
    """In the place of the model: prepared posteriors and attention of a run's windows as leaves of the graph."""

    def __init__(self, strong, att):
        self.strong, self.att = strong, att

    def __call__(self, x, return_attention=False):
        assert return_attention and x.shape[0] == self.strong.shape[0]
        return self.strong, None, self.att


def test_unknown_targets_take_no_part_in_the_loss():
    """Run (0, 2) of the small set: recordings of 8 and 12 label frames, span3 = 4 -> spans 0 .. 4 of the set.  Span 1 is all
    unknown, span 3 is known in one class only, some known targets are exactly 0 and 1.

    The value against float64 numpy on the kernel's own float32 tags x: l = -(t log x + (1 - t) log(1 - x)) over the n known
    pairs, loss = sum l / n.  Bound, from the formats (eps = 2^-24, a float32 half-ulp): per term the two logs at 1 ulp (2 eps
    each of its product), the product and the final subtraction one rounding each - 4 eps (|t log x| + |(1 - t) log(1 - x)|) -
    and the rounding of 1 - x, eps (1 - t) / (1 - x); the float32 sum of the N masked terms in any order, (N - 1) eps sum l;
    the division by N, the float32 scale N / n and the product with it, 3 eps of the loss; and one float32 step of the loss
    for the last bit."""
    from dcase2019_task4_amd.inference import span_table, stitch_span_tags
    from dcase2019_task4_amd.train import span_tag_plan, span_tags_loss
    ls = _small_set()
    span3 = 4
    rs = np.random.RandomState(196)
    host, dev_table, total, _ = span_table(ls, span3)
    assert host.tolist() == [0, 2, 5, 9]
    t = rs.uniform(size=(total, NCLS)).astype(np.float32)
    t[0, :3] = 0.0
    t[2, :3] = 1.0
    t[1] = np.nan
    t[3, 1:] = np.nan
    t[6] = np.nan                                                                  # (run 1)
    plan = span_tag_plan(ls.rec_win0_host, ls.rec_frame0_host, t, 4, span3)
    assert plan["runs"] == [(0, 2), (2, 3)] and plan["counts"].tolist() == [3 * NCLS + 1, 3 * NCLS]
    runs, at, win0_all, frame0_all = ls.tag_batches(4)
    span0_all = torch.from_numpy(np.concatenate([host[r0:r1 + 1] - host[r0] for r0, r1 in runs])).cuda()
    p, a = _inputs(rs, 3, 8, NCLS)
    strong, att = torch.from_numpy(p).cuda().requires_grad_(True), torch.from_numpy(a).cuda().requires_grad_(True)
    loss, err = span_tags_loss(ls, torch.from_numpy(plan["targets"]).cuda(), torch.from_numpy(plan["known"]).cuda(),
                               _Heads(strong, att), runs[0], (0, at, win0_all, frame0_all, span0_all, host, plan["counts"]), span3)
    loss.backward()
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    # the frames of span 1 (recording 0, frames 4 .. 7 of its one window) get no gradient; the others do
    ds, da = strong.grad.cpu().numpy(), att.grad.cpu().numpy()
    assert not ds[0, 4:].any() and not da[0, 4:].any() and ds[0, :4].all() and da[0, :4].any()
    # span 3 = frames 4 .. 7 of recording 1 (windows 1 and 2 at hop3 = 4): class 0 only
    assert not ds[1, 4:, 1:].any() and not ds[2, :4, 1:].any() and ds[1, 4:, 0].all() and ds[2, :4, 0].all()
    assert not da[1, 4:, 1:].any() and not da[2, :4, 1:].any()
    assert ds[1, :4].all() and ds[2, 4:].all()
    # the value
    w0, f0 = win0_all[at[0]:at[1]], frame0_all[at[0]:at[1]]
    x = stitch_span_tags(strong.detach(), att.detach(), w0, f0, 20, ls.hop3, span3, rec_frame0_host=[0, 8, 20])["tags"]
    x = x.cpu().numpy().astype(np.float64)
    tt = t[:5].astype(np.float64)
    known = ~np.isnan(tt)
    n, N, eps = int(known.sum()), tt.size, 2.0 ** -24
    assert n == plan["counts"][0]
    with np.errstate(all="ignore"):
        la, lb = np.where(known, -tt * np.log(x), 0.0), np.where(known, -(1 - tt) * np.log(1 - x), 0.0)
        slack = np.where(known, (1 - tt) / (1 - x), 0.0)
    want = float((la + lb).sum() / n)
    bound = (4 * eps * float((np.abs(la) + np.abs(lb)).sum()) + eps * float(slack.sum()) + (N - 1) * eps * float((la + lb).sum())) / n \
        + 3 * eps * want + float(np.spacing(np.float32(want)))
    got = float(loss.detach())
    print(f"span_tags_loss {got!r} against float64 {want!r}: |difference| {abs(got - want):.3e}, bound {bound:.3e}")
    assert abs(got - want) <= bound


def _epoch(train_fn, state, ls, *args, **kw):
    """One epoch on a fresh model of the given parameters under one torch seed (the dropout stream's base is drawn from it):
    (the parameters afterwards as bytes, the mean loss)."""
    model, _ = gu.make_model(0)
    model.load(parameters=state)
    torch.manual_seed(1234)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    mean = train_fn(ls, *args, model, opt, 0, max_windows=4, seed=5, **kw)
    torch.cuda.synchronize()
    model.flatten_parameters_()
    return model._flat.detach().cpu().numpy().tobytes(), mean


def test_an_epoch_on_one_span_per_recording_is_train_recording_tags_bit_for_bit():
    """T = 64 frames per window, recordings of 1, 2 and 3 windows, max_windows 4 (two batches), dropout at the model's default.
    With span3 >= the longest recording the epoch is train_recording_tags' operation for operation: bit-equal parameters.  With
    span3 = 4 and distinct tags per span the parameters differ and the epoch's error word is zero (it would raise)."""
    from dcase2019_task4_amd.train import train_recording_tags, train_span_tags
    ls = _small_set()
    first, _ = gu.make_model(0)
    state = copy.deepcopy(first.state_dict())
    first.flatten_parameters_()
    start = first._flat.detach().cpu().numpy().tobytes()
    tags = np.random.RandomState(197).uniform(size=(3, NCLS)).astype(np.float32)
    want, want_mean = _epoch(train_recording_tags, state, ls, tags)
    assert want != start
    for kw in (dict(span3=16), dict(span3=1000), dict(tag_span=float("inf"))):
        got, mean = _epoch(train_span_tags, state, ls, tags, **kw)
        assert got == want and mean == want_mean, kw
    span_tags = np.random.RandomState(198).uniform(size=(9, NCLS)).astype(np.float32)
    span_tags[4] = np.nan
    got, mean = _epoch(train_span_tags, state, ls, span_tags, span3=4)
    assert got != want and got != start and 0 < mean < 1e5
    # seconds: 4 label frames of 8 * 511 / 44100 s fit into 0.4 s (and 5 do not)
    assert _epoch(train_span_tags, state, ls, span_tags, tag_span=0.4) == (got, mean)
    # a batch without a known pair is skipped: the epoch is the epoch of the other batch alone
    half = span_tags.copy()
    half[5:] = np.nan
    only_first, _ = _epoch(train_span_tags, state, ls, half, span3=4)
    assert only_first != start and only_first != got

"""-m gpu tests of span tags in pieces: sed_stitch_piece_span_tags / sed_stitch_piece_span_tags_backward over the pieces of
longrec.span_pieces against ONE span call over the whole recordings' windows (bit for bit) and against the plain-loop statement,
the span entries' bytes at off = 0, aligned / misaligned / repeated / graph-replayed calls, inference.pooled_span_tags with
span_off against the direct calls, the error bits of a malformed piece, and epochs of train.train_span_tags(split_long=True).
Every buffer a kernel writes starts as NaN / 0xFF bytes and carries a tail that must come back untouched."""
import copy

import numpy as np
import pytest
import torch

from tests import gpu_util as gu
from tests import span_pieces_np as pn
from tests import span_tags_np, stitch_np
from tests.long_util import _Scaler, _tile
from tests.test_gpu_long import _recordings
from tests.test_gpu_span_tags import SpanCall, _check, _inputs
from tests.test_gpu_span_tags_bwd import SpanBwdCall, _g
from tests.test_span_pieces_cpu import HOPS, SPANS, T3, TILE, WINDOWS, lengths, min_windows

pytestmark = pytest.mark.gpu


class PieceCall(SpanCall):
    """One sed_stitch_piece_span_tags call on SpanCall's sentinel-filled outputs."""

    def __init__(self, p, a, rec_win0, rec_frame0, rec_span0, rec_span_off, hop3, weighting, span3, misalign=None, total_spans=None):
        super().__init__(p, a, rec_win0, rec_frame0, hop3, weighting, span3, misalign, rec_span0, total_spans)
        self.rec_span_off = torch.from_numpy(np.asarray(rec_span_off, dtype=np.int32)).cuda()
        assert self.ws_bytes == self.l.sed_stitch_piece_span_tags_ws_bytes(self.total, self.total_spans, self.n_rec, self.NC, self.span3)

    def launch(self, **kw):
        ptr = self._lib.ptr
        a = dict(p=self.p, a=self.a, span0=self.rec_span0, off=self.rec_span_off, total=self.total, total_spans=self.total_spans,
                 n_rec=self.n_rec, T3=self.T3, NC=self.NC, hop3=self.hop3, weighting=self.weighting, span3=self.span3, weak=self.weak,
                 sums=self.sums, ws=self.ws, ws_bytes=self.ws_bytes)
        a.update(kw)
        return self.l.sed_stitch_piece_span_tags(ptr(a["p"]), ptr(a["a"]), ptr(self.rec_win0), ptr(self.rec_frame0), ptr(a["span0"]),
                                                 a["total"], a["total_spans"], a["n_rec"], a["T3"], a["NC"], a["hop3"],
                                                 a["weighting"], a["span3"], ptr(a["off"]), ptr(a["weak"]), ptr(a["sums"]),
                                                 ptr(a["ws"]), a["ws_bytes"], ptr(self.err), self._lib.stream_ptr())


class PieceBwdCall(SpanBwdCall):
    """One sed_stitch_piece_span_tags_backward call on SpanBwdCall's 0xFF-filled outputs."""

    def __init__(self, p, a, rec_win0, rec_frame0, rec_span0, rec_span_off, hop3, weighting, span3, g, sums, misalign=None,
                 total_spans=None):
        super().__init__(p, a, rec_win0, rec_frame0, hop3, weighting, span3, g, sums, misalign, rec_span0, total_spans)
        self.rec_span_off = torch.from_numpy(np.asarray(rec_span_off, dtype=np.int32)).cuda()

    def launch(self, **kw):
        ptr = self._lib.ptr
        k = dict(p=self.p, a=self.a, n_rec=self.n_rec, T3=self.T3, NC=self.NC, hop3=self.hop3, weighting=self.weighting,
                 span3=self.span3, total_spans=self.total_spans, sums=self.sums, g=self.g, ds=self.ds, da=self.da, err=self.err,
                 w0=self.rec_win0, f0=self.rec_frame0, s0=self.rec_span0, off=self.rec_span_off)
        k.update(kw)
        return self.l.sed_stitch_piece_span_tags_backward(ptr(k["p"]), ptr(k["a"]), ptr(k["w0"]), ptr(k["f0"]), ptr(k["s0"]),
                                                          k["total_spans"], k["n_rec"], k["T3"], k["NC"], k["hop3"], k["weighting"],
                                                          k["span3"], ptr(k["off"]), ptr(k["sums"]), ptr(k["g"]), ptr(k["ds"]),
                                                          ptr(k["da"]), ptr(k["err"]), self._lib.stream_ptr())


def _whole_tables(windows, L3s):
    return np.r_[0, np.cumsum(windows)].astype(np.int32), np.r_[0, np.cumsum(L3s)].astype(np.int64)


def _piece_set(windows, L3s, hop3, span3, max_windows):
    """All pieces of an epoch as the "recordings" of ONE call: (pieces, window indices of the whole set that the call's window
    tensor gathers - boundary windows twice -, rec_win0, rec_frame0, rec_span0, rec_span_off).  The pieces come in recording and
    span order, so row g of the call is row g of the whole recordings' span table."""
    from dcase2019_task4_amd.longrec import span_pieces
    win0 = np.r_[0, np.cumsum(windows)]
    pieces = [p for b in span_pieces(windows, L3s, T3, hop3, span3, max_windows) for p in b]
    idx = np.concatenate([np.arange(win0[p.rec] + p.j0, win0[p.rec] + p.j1 + 1) for p in pieces])
    return (pieces, idx, np.r_[0, np.cumsum([p.j1 - p.j0 + 1 for p in pieces])].astype(np.int32),
            np.r_[0, np.cumsum([p.L3 for p in pieces])].astype(np.int64),
            np.r_[0, np.cumsum([p.s1 - p.s0 for p in pieces])].astype(np.int64), np.array([p.off for p in pieces], np.int32))


def _configs(windows, L3s, hop3):
    for span3 in SPANS:
        lo = min_windows(windows, L3s, hop3, span3)
        for max_windows in sorted({lo, 4, 6}):
            if max_windows >= lo:
                yield span3, max_windows


def _compare(p, a, windows, L3s, hop3, weighting, span3, max_windows, misalign, rs, statement=True):
    """Forward and backward of all pieces in one call each against one span call over the whole recordings."""
    NC = p.shape[2]
    rec_win0, rec_frame0 = _whole_tables(windows, L3s)
    whole = SpanCall(p, a, rec_win0, rec_frame0, hop3, weighting, span3, misalign).run()
    assert whole["err"] == 0
    pieces, idx, w0, f0, s0, off = _piece_set(windows, L3s, hop3, span3, max_windows)
    what = f"hop3 {hop3} weighting {weighting} NC {NC} span3 {span3} max_windows {max_windows}: {len(pieces)} pieces"
    got = PieceCall(p[idx], a[idx], w0, f0, s0, off, hop3, weighting, span3, misalign).run()
    assert got["err"] == 0, what
    assert got["tags"].tobytes() == whole["tags"].tobytes() and got["sums"].tobytes() == whole["sums"].tobytes(), what
    if statement:
        P, A = stitch_np.blend(p, rec_win0, rec_frame0, hop3, weighting), stitch_np.blend(a, rec_win0, rec_frame0, hop3, weighting)
        want_tags, want_sums, _ = span_tags_np.pool_timelines(P, A, rec_frame0, span3)
        _check(got, want_tags, want_sums, [min(span3, L - s * span3) for L in L3s for s in range(-(-L // span3))], what)
    # backward: the whole call on the whole windows, the piece call on the gathered ones
    g = _g(rs, len(whole["sums"]), NC)
    bm = {"p": "ds", "a": "da"}.get(misalign)
    wb = SpanBwdCall(p, a, rec_win0, rec_frame0, hop3, weighting, span3, g, whole["sums"], bm).run()
    pb = PieceBwdCall(p[idx], a[idx], w0, f0, s0, off, hop3, weighting, span3, g, got["sums"], bm).run()
    assert wb["err"] == 0 and pb["err"] == 0, what
    row, _ = pn.frame_rows(w0, f0, s0, off, T3, hop3, weighting, span3)
    owned = row >= 0
    g_at = np.where(owned[:, :, None], g[np.maximum(row, 0)], 0.0)
    zero = np.zeros(1, np.float32).tobytes()
    n_owned = 0
    for name in ("ds", "da"):
        mine, theirs = pb[name], wb[name][idx]
        live = owned[:, :, None] & (g_at != 0)
        assert mine[live].tobytes() == theirs[live].tobytes(), (what, name)
        assert (mine[~live] == 0).all(), (what, name)
        assert mine[~owned].tobytes() == zero * int((~owned).sum()) * NC, (what, name)         # no span's frames and tails: +0.0f
        total = np.zeros_like(wb[name])
        np.add.at(total, idx, mine)
        assert (total == wb[name]).all(), (what, name)
        n_owned += int(live.sum())
    assert n_owned > 0 and (owned.sum(axis=None) > 0)
    # a window element of the whole set is owned by exactly one piece, or by none (the recordings' tails)
    owners = np.zeros(int(rec_win0[-1]) * T3, np.int64)
    np.add.at(owners, (idx[:, None] * T3 + np.arange(T3)[None, :])[owned], 1)
    tails = np.zeros((int(rec_win0[-1]), T3), bool)
    for r, L3 in enumerate(L3s):
        for j in range(windows[r]):
            tails[rec_win0[r] + j, max(0, L3 - j * hop3):] = True
    assert (owners.reshape(-1, T3) == ~tails).all(), what
    return len(pieces)


@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", HOPS)
@pytest.mark.parametrize("NC,misalign", [(10, None), (8, None), (8, "p"), (8, "a")])
def test_pieces_give_the_whole_recordings_bits_forward_and_backward(NC, misalign, hop3, weighting):
    """Recordings of 1, 2, 7 and 23 windows with a short last window; span3 in {1, 3, 5, 8, 13} x max_windows in {the fewest
    the plan accepts, 4, 6} (those of them the plan accepts).  Tags and sums: bit-equal to the rows of one sed_stitch_span_tags
    call over the whole recordings, and within the span test's bounds of the statement (one fp32 step, (len - 1) 2^-53 relative).
    Backward: the whole call's bytes wherever the piece owns the frame and g != 0, == 0 elsewhere, +0.0f on frames of no span and
    tails, and the sum over the pieces is the whole call."""
    assert _tile() == TILE
    L3s = lengths(hop3)
    rs = np.random.RandomState(900 + 10 * hop3 + weighting + NC)
    p, a = _inputs(rs, sum(WINDOWS), T3, NC)
    n = [_compare(p, a, WINDOWS, L3s, hop3, weighting, span3, m, misalign, rs, statement=misalign is None)
         for span3, m in _configs(WINDOWS, L3s, hop3)]
    assert len(n) >= 10 and max(n) > 10


@pytest.mark.parametrize("NC", [8, 10])
def test_a_span_longer_than_a_tile_in_pieces(NC):
    """span3 = tile + 1 (two tiles per span, the second of one frame), hop3 = 4, 300 windows, max_windows 140."""
    hop3, span3 = 4, _tile() + 1
    L3s = lengths(hop3, [300])
    rs = np.random.RandomState(950 + NC)
    p, a = _inputs(rs, 300, T3, NC)
    assert _compare(p, a, [300], L3s, hop3, 1, span3, 140, None, rs) == 3


@pytest.mark.parametrize("NC,misalign", [(10, None), (8, None), (8, "a")])
def test_off_zero_and_all_spans_is_the_span_entries_bytes(NC, misalign):
    hop3, weighting = 3, 1
    L3s = lengths(hop3)
    rec_win0, rec_frame0 = _whole_tables(WINDOWS, L3s)
    rs = np.random.RandomState(960 + NC)
    p, a = _inputs(rs, sum(WINDOWS), T3, NC)
    for span3 in SPANS + [max(L3s)]:
        span0 = span_tags_np.span_table(L3s, span3)
        off = np.zeros(len(L3s), np.int32)
        want = SpanCall(p, a, rec_win0, rec_frame0, hop3, weighting, span3, misalign).run()
        got = PieceCall(p, a, rec_win0, rec_frame0, span0, off, hop3, weighting, span3, misalign).run()
        assert want["err"] == got["err"] == 0
        assert got["tags"].tobytes() == want["tags"].tobytes() and got["sums"].tobytes() == want["sums"].tobytes()
        g = _g(rs, len(want["sums"]), NC)
        bm = {"a": "da"}.get(misalign)
        wb = SpanBwdCall(p, a, rec_win0, rec_frame0, hop3, weighting, span3, g, want["sums"], bm).run()
        pb = PieceBwdCall(p, a, rec_win0, rec_frame0, span0, off, hop3, weighting, span3, g, want["sums"], bm).run()
        assert wb["err"] == pb["err"] == 0 and wb["ds"].any()
        assert pb["ds"].tobytes() == wb["ds"].tobytes() and pb["da"].tobytes() == wb["da"].tobytes()


def _one_set(NC, hop3=3, span3=5, max_windows=4, seed=970):
    L3s = lengths(hop3)
    rs = np.random.RandomState(seed + NC)
    p, a = _inputs(rs, sum(WINDOWS), T3, NC)
    pieces, idx, w0, f0, s0, off = _piece_set(WINDOWS, L3s, hop3, span3, max_windows)
    return p[idx], a[idx], w0, f0, s0, off, hop3, span3, rs


def test_aligned_misaligned_repeated_and_replayed_calls_give_identical_bytes():
    NC, weighting = 8, 1
    p, a, w0, f0, s0, off, hop3, span3, rs = _one_set(NC)
    call = PieceCall(p, a, w0, f0, s0, off, hop3, weighting, span3)
    first = call.run()
    assert first["err"] == 0 and not np.isnan(first["tags"]).any()
    g = _g(rs, len(first["sums"]), NC)
    bwd = PieceBwdCall(p, a, w0, f0, s0, off, hop3, weighting, span3, g, first["sums"])
    bfirst = bwd.run()
    assert bfirst["err"] == 0 and bfirst["ds"].any() and bfirst["da"].any()
    for mis in ("p", "a"):
        other = PieceCall(p, a, w0, f0, s0, off, hop3, weighting, span3, mis).run()
        assert other["tags"].tobytes() == first["tags"].tobytes() and other["sums"].tobytes() == first["sums"].tobytes(), mis
    for mis in ("p", "a", "ds", "da"):
        other = PieceBwdCall(p, a, w0, f0, s0, off, hop3, weighting, span3, g, first["sums"], mis).run()
        assert other["err"] == 0 and other["ds"].tobytes() == bfirst["ds"].tobytes() and other["da"].tobytes() == bfirst["da"].tobytes(), mis
    for c, ref, keys in ((call, first, ("tags", "sums")), (bwd, bfirst, ("ds", "da"))):
        second = c.run()
        graph = torch.cuda.CUDAGraph()
        c.fill()
        with torch.cuda.graph(graph):
            assert c.launch() == 0
        c.fill()
        graph.replay()
        third = c.get()
        for other in (second, third):
            assert other["err"] == 0 and all(other[k].tobytes() == ref[k].tobytes() for k in keys)


@pytest.mark.parametrize("NC", [10, 8])
def test_pooled_span_tags_with_span_off_is_the_direct_calls(NC):
    from dcase2019_task4_amd.inference import pooled_span_tags, stitch_span_tags
    weighting = 1
    p, a, w0, f0, s0, off, hop3, span3, rs = _one_set(NC, seed=980)
    tp, ta = torch.from_numpy(p).cuda().requires_grad_(True), torch.from_numpy(a).cuda().requires_grad_(True)
    dw0, df0, ds0, doff = (torch.from_numpy(x).cuda() for x in (w0, f0, s0, off))
    out = pooled_span_tags(tp, ta, dw0, df0, int(f0[-1]), hop3, span3, n_win=int(w0[-1]), rec_frame0_host=f0,
                           span_tables=(s0, ds0), span_off=doff)
    plain = stitch_span_tags(tp.detach(), ta.detach(), dw0, df0, int(f0[-1]), hop3, span3, want_sums=True, rec_frame0_host=f0,
                             span_tables=(s0, ds0), span_off=(off, doff))
    fwd = PieceCall(p, a, w0, f0, s0, off, hop3, weighting, span3).run()
    assert out["total_spans"] == plain["total_spans"] == int(s0[-1]) and out["span3"] == span3
    assert out["tags"].requires_grad and torch.equal(out["tags"].detach(), plain["tags"])
    assert plain["tags"].cpu().numpy().tobytes() == fwd["tags"].tobytes() and plain["sums"].cpu().numpy().tobytes() == fwd["sums"].tobytes()
    g = _g(rs, int(s0[-1]), NC)
    out["tags"].backward(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    assert int(out["err"].item()) == 0 and int(plain["err"].item()) == 0
    want = PieceBwdCall(p, a, w0, f0, s0, off, hop3, weighting, span3, g, fwd["sums"]).run()
    assert want["err"] == 0 and want["ds"].any() and want["da"].any()
    assert tp.grad.cpu().numpy().tobytes() == want["ds"].tobytes() and ta.grad.cpu().numpy().tobytes() == want["da"].tobytes()
    # what the host refuses
    with pytest.raises(ValueError, match="span_off needs span_tables"):
        pooled_span_tags(tp, ta, dw0, df0, int(f0[-1]), hop3, span3, rec_frame0_host=f0, span_off=doff)
    with pytest.raises(ValueError, match="do not describe pieces"):
        pooled_span_tags(tp, ta, dw0, df0, int(f0[-1]), hop3, span3, rec_frame0_host=f0, span_tables=(s0, ds0), span_off=(off - 1, doff))
    with pytest.raises(ValueError, match="int32"):
        pooled_span_tags(tp, ta, dw0, df0, int(f0[-1]), hop3, span3, rec_frame0_host=f0, span_tables=(s0, ds0), span_off=(off, doff.long()))


# ---- a malformed piece ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NC", [10, 8])
@pytest.mark.parametrize("case", ["off_negative", "last_span_empty", "no_span", "beyond_total"])
def test_a_malformed_piece_raises_bit_16_and_only_its_rows_and_windows_are_lost(case, NC):
    """Three pieces of 3 windows (hop3 = 3: 14 local frames), two spans of 5 frames each from off 1, 2 and 3.  One piece's
    entries are broken; its rows are NaN and its windows +0.0f, the other pieces' rows and windows are the clean call's."""
    hop3, weighting, span3 = 3, 1, 5
    w0, f0 = np.array([0, 3, 6, 9], np.int32), np.array([0, 14, 28, 42], np.int64)
    s0, off = np.array([0, 2, 4, 6], np.int64), np.array([1, 2, 3], np.int32)
    rs = np.random.RandomState(990 + NC)
    p, a = _inputs(rs, 9, T3, NC)
    clean = PieceCall(p, a, w0, f0, s0, off, hop3, weighting, span3).run()
    assert clean["err"] == 0 and not np.isnan(clean["tags"]).any()
    g = _g(rs, 6, NC)
    g[g == 0] = 0.5
    cb = PieceBwdCall(p, a, w0, f0, s0, off, hop3, weighting, span3, g, clean["sums"]).run()
    assert cb["err"] == 0
    bs0, boff, total, bad = s0.copy(), off.copy(), 6, 1
    if case == "off_negative":
        boff[1] = -1
    elif case == "last_span_empty":
        boff[1] = 9                                                                # 9 + 1 * 5 >= 14
    elif case == "no_span":
        bs0 = np.array([0, 2, 2, 4], np.int64)
        total = 4
    else:
        total, bad = 5, 2                                                          # the last piece's rows reach beyond the total
    good = [r for r in range(3) if r != bad]
    n_rows = min(total, int(bs0[-1]))
    # sums and g of the broken call: the clean rows of the good pieces at their rows of the broken table
    bsums, bg = np.ones((max(total, int(bs0[-1])), NC, 2)), np.ones((max(total, int(bs0[-1])), NC), np.float32)
    for r in good:
        bsums[bs0[r]:bs0[r + 1]], bg[bs0[r]:bs0[r + 1]] = clean["sums"][s0[r]:s0[r + 1]], g[s0[r]:s0[r + 1]]
    got = PieceCall(p, a, w0, f0, bs0, boff, hop3, weighting, span3, total_spans=total).run()
    assert got["err"] == 16 and got["tags"].shape[0] == total
    for r in good:
        assert got["tags"][bs0[r]:bs0[r + 1]].tobytes() == clean["tags"][s0[r]:s0[r + 1]].tobytes(), r
        assert got["sums"][bs0[r]:bs0[r + 1]].tobytes() == clean["sums"][s0[r]:s0[r + 1]].tobytes(), r
    lost = [x for x in range(n_rows) if not any(bs0[r] <= x < bs0[r + 1] for r in good)]
    assert np.isnan(got["tags"][lost]).all() and np.isnan(got["sums"][lost]).all() and (case == "no_span" or lost)
    gb = PieceBwdCall(p, a, w0, f0, bs0, boff, hop3, weighting, span3, bg, bsums, total_spans=total).run()
    assert gb["err"] == 16
    zero = np.zeros(3 * T3 * NC, np.float32).tobytes()
    for name in ("ds", "da"):
        assert gb[name][w0[bad]:w0[bad + 1]].tobytes() == zero, name
        for r in good:
            assert gb[name][w0[r]:w0[r + 1]].tobytes() == cb[name][w0[r]:w0[r + 1]].tobytes() and gb[name][w0[r]:w0[r + 1]].any(), (name, r)


@pytest.mark.parametrize("NC", [4, 3])
def test_one_table_short_of_the_ceiling_is_malformed_for_spans_and_a_piece_at_off_zero(NC):
    """The span entries and the piece entries run the same kernels; only rec_span_off (null or not) tells them apart.  Recordings
    of 23 and 12 frames (5 and 2 windows, hop3 = 4, taper), span3 = 4, rec_span0 = [0, 4, 7]: recording 0 is given 4 spans where
    the ceiling is 6, recording 1 its 3.  The span entries reject recording 0 (bit 16, NaN rows, +0.0f windows); the piece
    entries at off = [0, 0] take it: its four spans are the first four of the clean call and its frames from 16 on own no span.
    Recording 1 is the clean call's in both.  NC = 4 takes the 16-byte path, NC = 3 the scalar one."""
    hop3, weighting, span3 = 4, 1, 4
    w0, f0 = np.array([0, 5, 7], np.int32), np.array([0, 23, 35], np.int64)
    s0, off = np.array([0, 4, 7], np.int64), np.zeros(2, np.int32)
    rs = np.random.RandomState(995 + NC)
    p, a = _inputs(rs, 7, T3, NC)
    clean = SpanCall(p, a, w0, f0, hop3, weighting, span3).run()
    assert clean["err"] == 0 and clean["tags"].shape[0] == 9 and not np.isnan(clean["tags"]).any()
    g = _g(rs, 9, NC)
    g[g == 0] = 0.5
    cb = SpanBwdCall(p, a, w0, f0, hop3, weighting, span3, g, clean["sums"]).run()
    assert cb["err"] == 0
    rows = np.r_[0:4, 6:9]                                                         # the clean rows behind the table's seven
    frame = 4 * np.arange(5)[:, None] + np.arange(T3)[None, :]                     # recording 0: the frame of window element (j, v)
    zero = np.zeros(1, np.float32).tobytes()
    # the span entries: recording 0 is malformed
    got = SpanCall(p, a, w0, f0, hop3, weighting, span3, rec_span0=s0).run()
    assert got["err"] == 16 and got["tags"].shape[0] == 7
    assert np.isnan(got["tags"][:4]).all() and np.isnan(got["sums"][:4]).all()
    assert got["tags"][4:].tobytes() == clean["tags"][6:].tobytes() and got["sums"][4:].tobytes() == clean["sums"][6:].tobytes()
    bsums, bg = np.ones((7, NC, 2)), np.ones((7, NC), np.float32)
    bsums[4:], bg[4:] = clean["sums"][6:], g[6:]
    gb = SpanBwdCall(p, a, w0, f0, hop3, weighting, span3, bg, bsums, rec_span0=s0).run()
    assert gb["err"] == 16
    for name in ("ds", "da"):
        assert gb[name][:5].tobytes() == zero * (5 * T3 * NC), name
        assert gb[name][5:].tobytes() == cb[name][5:].tobytes() and gb[name][5:].any(), name
    # the piece entries: the same tables describe a piece of four spans and the whole of recording 1
    got = PieceCall(p, a, w0, f0, s0, off, hop3, weighting, span3).run()
    assert got["err"] == 0 and got["tags"].shape[0] == 7
    assert got["tags"].tobytes() == clean["tags"][rows].tobytes() and got["sums"].tobytes() == clean["sums"][rows].tobytes()
    gb = PieceBwdCall(p, a, w0, f0, s0, off, hop3, weighting, span3, g[rows], clean["sums"][rows]).run()
    assert gb["err"] == 0
    for name in ("ds", "da"):
        assert gb[name][:5][frame >= 16].tobytes() == zero * (int((frame >= 16).sum()) * NC), name
        assert gb[name][:5][frame < 16].tobytes() == cb[name][:5][frame < 16].tobytes() and gb[name][:5][frame < 16].any(), name
        assert gb[name][5:].tobytes() == cb[name][5:].tobytes() and gb[name][5:].any(), name


def test_bad_host_arguments_return_before_any_launch():
    p, a, w0, f0, s0, off, hop3, span3, rs = _one_set(10)
    call = PieceCall(p, a, w0, f0, s0, off, hop3, 1, span3)
    call.fill()
    for kw in (dict(off=None), dict(span0=None), dict(span3=0), dict(NC=17), dict(hop3=9), dict(ws_bytes=call.ws_bytes - 16),
               dict(total_spans=call.n_rec - 1)):
        assert call.launch(**kw) == -1, kw
    assert call.untouched()
    first = call.run()
    bwd = PieceBwdCall(p, a, w0, f0, s0, off, hop3, 1, span3, _g(rs, len(first["sums"]), 10), first["sums"])
    bwd.fill()
    for kw in (dict(off=None), dict(s0=None), dict(span3=0), dict(NC=17), dict(total_spans=call.n_rec - 1)):
        assert bwd.launch(**kw) == -1, kw
    assert bwd.untouched()


# ---- the epoch -------------------------------------------------------------------------------------------------------------------------
FR, HOP, NCLS = 64, 32, 10


def _set(lengths_):
    from dcase2019_task4_amd.inference import LongRecordingSet
    ls = LongRecordingSet.from_arrays(_recordings(lengths_), FR, hop_frames=HOP, scaler=_Scaler(64))
    assert ls.T3 == 8 and ls.hop3 == 4
    return ls


def _epoch(state, ls, span_tags, span3, max_windows, **kw):
    """One train_span_tags epoch on a fresh model of the given parameters under one torch seed: (the parameters afterwards as
    bytes, the mean loss, the optimizer steps taken)."""
    from dcase2019_task4_amd.train import train_span_tags
    model, _ = gu.make_model(0)
    model.load(parameters=state)
    torch.manual_seed(1234)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    steps, step = [], opt.step

    def counted(*args, **kwargs):
        steps.append(1)
        return step(*args, **kwargs)

    opt.step = counted
    mean = train_span_tags(ls, span_tags, model, opt, 0, span3=span3, max_windows=max_windows, seed=5, **kw)
    torch.cuda.synchronize()
    model.flatten_parameters_()
    return model._flat.detach().cpu().numpy().tobytes(), mean, len(steps)


def _state():
    first, _ = gu.make_model(0)
    state = copy.deepcopy(first.state_dict())
    first.flatten_parameters_()
    return state, first._flat.detach().cpu().numpy().tobytes()


def test_an_epoch_without_a_long_recording_is_todays_epoch_bit_for_bit():
    """Recordings of 1, 2 and 3 windows, max_windows 4, dropout at the model's default: split_long=True goes through the piece
    entries with off = 0 and leaves bit-equal parameters."""
    ls = _set([64, 96, 128])
    state, start = _state()
    t = np.random.RandomState(198).uniform(size=(9, NCLS)).astype(np.float32)
    t[4] = np.nan
    want = _epoch(state, ls, t, 4, 4)
    got = _epoch(state, ls, t, 4, 4, split_long=True)
    assert want[0] != start and got == want and want[2] == 2


def test_an_epoch_over_a_23_window_recording_in_pieces():
    """Recordings of 1, 23 and 2 windows at max_windows 6, span3 = 5: the long one is trained in pieces."""
    from dcase2019_task4_amd.inference import span_table
    from dcase2019_task4_amd.train import span_tag_plan, train_span_tags
    ls = _set([64, 760, 96])
    assert list(np.diff(ls.rec_win0_host)) == [1, 23, 2] and list(np.diff(ls.rec_frame0_host)) == [8, 95, 12]
    state, start = _state()
    host, _, total, span3 = span_table(ls, 5)
    t = np.random.RandomState(199).uniform(size=(total, NCLS)).astype(np.float32)
    with pytest.raises(ValueError, match="more than max_windows = 6"):
        train_span_tags(ls, t, None, None, 0, span3=5, max_windows=6)
    plan = span_tag_plan(ls.rec_win0_host, ls.rec_frame0_host, t, 6, 5, split_long=True, T3=ls.T3, hop3=ls.hop3)
    n_batches = len(plan["runs"])
    assert n_batches >= 6 and plan["ran"] == list(range(n_batches)) and plan["forwarded"] > 1
    first = _epoch(state, ls, t, 5, 6, split_long=True)
    assert first[0] != start and np.isfinite(first[1]) and 0 < first[1] < 1e5 and first[2] == n_batches
    assert _epoch(state, ls, t, 5, 6, split_long=True) == first
    # NaN targets that empty one piece skip exactly that batch
    k = [i for i, b in enumerate(plan["runs"]) if b[0].rec == 1][2]
    piece = plan["runs"][k][0]
    t2 = t.copy()
    t2[host[1] + piece.s0:host[1] + piece.s1] = np.nan
    plan2 = span_tag_plan(ls.rec_win0_host, ls.rec_frame0_host, t2, 6, 5, split_long=True, T3=ls.T3, hop3=ls.hop3)
    assert plan2["ran"] == [i for i in range(n_batches) if i != k]
    skipped = _epoch(state, ls, t2, 5, 6, split_long=True)
    assert skipped[2] == n_batches - 1 and skipped[0] != first[0] and np.isfinite(skipped[1])

"""-m gpu tests of sed_events_scores and sed_events_select against the plain-loop statement (tests/event_scores_np.py):
event lengths on both sides of the short / long edge and of a wave's stride, position edges, shapes and alignments, every
count of long events in a wave, workgroup edges, more than 1 024 workgroups, NaN frames, the error bits, two calls and one
graph replay, the cross-checks (K points = K calls, -inf keeps all, the select on the maximum = the two-threshold decode at
window 1, compacted scores = fresh scores, clip batches) and get_long_predictions.

Every output buffer starts as sentinel bytes (-7.0 / -7) and carries a tail that must come back untouched.  Maxima are
compared bitwise.  Means must lie within one fp32 step (np.spacing) of the statement, a bound that is derived, not measured:
the fp64 sum of n < 2^28 non-negative fp32 values is within (n - 1) * 2^-53 relative of the exact sum in any order, the
quotient is rounded once to fp64 and once to fp32; every posterior here is >= +0.0 or NaN, so nothing cancels."""
import functools

import numpy as np
import pytest
import torch

from tests import event_scores_np as es
from tests import gpu_util as gu
from tests.hysteresis_np import smooth_timeline
from tests.long_util import SENT, TAIL, StitchCall, _Scaler
from tests.test_event_scores_cpu import HYST_GRID, decode_points, hysteresis_case

pytestmark = pytest.mark.gpu

NUM, DEN = 8.0, 44100 / 511
BLOCK = 256                                                                    # indices per workgroup of the flat passes
SENTF = np.float32(SENT)


def _short():
    from dcase2019_task4_amd import _lib
    return int(_lib.lib().sed_events_scores_short_frames())


def _dev(a, dt):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


class ScoresCall:
    """One sed_events_scores call on sentinel-filled outputs with a tail of TAIL elements that ``get()`` checks; ``misalign``
    shifts the timeline off 16-byte alignment.  Arrays are numpy or device tensors; ``ev_pairs`` [capacity, 2]."""

    def __init__(self, tl, rec_frame0, NC, ev_ptr, ev_pairs, misalign=False):
        from dcase2019_task4_amd import _lib
        self._lib, self.l, self.NC = _lib, _lib.lib(), NC
        off = 1 if misalign else 0
        if torch.is_tensor(tl):
            assert not misalign
            self.tl = tl.contiguous().view(-1)
        else:
            tl = np.ascontiguousarray(tl, dtype=np.float32).reshape(-1)
            self._tl = torch.empty(tl.size + off + 1, dtype=torch.float32, device="cuda")
            self.tl = self._tl[off:off + tl.size]
            self.tl.copy_(torch.from_numpy(tl))
            assert (self.tl.data_ptr() % 16 != 0) == bool(misalign)
        self.total = self.tl.numel() // NC
        self.f0, self.ptr = _dev(rec_frame0, np.int64), _dev(ev_ptr, np.int64)
        self.pairs = _dev(ev_pairs if torch.is_tensor(ev_pairs) else np.asarray(ev_pairs).reshape(-1, 2), np.int32)
        self.n_rec, self.n_cols, self.cap = self.f0.numel() - 1, self.ptr.numel() - 1, self.pairs.shape[0]
        if self.cap == 0:
            self.pairs = torch.full((1, 2), SENT, dtype=torch.int32, device="cuda")              # (an address; no row is given)
        self.smax = torch.empty(self.cap + TAIL, dtype=torch.float32, device="cuda")
        self.smean = torch.empty(self.cap + TAIL, dtype=torch.float32, device="cuda")
        self.err = torch.empty(2, dtype=torch.int32, device="cuda")

    def fill(self, err0=0):
        self.smax.fill_(float(SENT))
        self.smean.fill_(float(SENT))
        self.err.fill_(SENT)
        self.err[:1].fill_(err0)

    def launch(self, **kw):
        p = self._lib.ptr
        a = dict(tl=self.tl, total=self.total, f0=self.f0, n_rec=self.n_rec, NC=self.NC, ptr=self.ptr, pairs=self.pairs,
                 cap=self.cap, n_cols=self.n_cols, smax=self.smax, smean=self.smean, err=self.err)
        a.update(kw)
        return self.l.sed_events_scores(p(a["tl"]), a["total"], p(a["f0"]), a["n_rec"], a["NC"], p(a["ptr"]), p(a["pairs"]),
                                        a["cap"], a["n_cols"], p(a["smax"]), p(a["smean"]), p(a["err"]), self._lib.stream_ptr())

    def get(self):
        torch.cuda.synchronize()
        smax, smean = self.smax.cpu().numpy(), self.smean.cpu().numpy()
        assert (smax[self.cap:] == SENTF).all() and (smean[self.cap:] == SENTF).all() and int(self.err[1].item()) == SENT
        return smax[:self.cap], smean[:self.cap], int(self.err[0].item())

    def run(self, err0=0, **kw):
        self.fill(err0)
        assert self.launch(**kw) == 0, self.l.sed_last_error()
        return self.get()


class SelectCall:
    """One sed_events_select call on sentinel-filled outputs and a 0xFF workspace, each with a tail ``get()`` checks."""

    def __init__(self, ev_ptr, ev_pairs, score_max, score_mean, n_rec, NC, min_score, key=0, out_capacity=None):
        from dcase2019_task4_amd import _lib
        self._lib, self.l, self.n_rec, self.NC, self.key = _lib, _lib.lib(), n_rec, NC, key
        self.ptr = _dev(ev_ptr, np.int64)
        self.pairs = _dev(ev_pairs if torch.is_tensor(ev_pairs) else np.asarray(ev_pairs).reshape(-1, 2), np.int32)
        self.n_cols, self.cap = self.ptr.numel() - 1, self.pairs.shape[0]
        if self.cap == 0:
            self.pairs = torch.full((1, 2), SENT, dtype=torch.int32, device="cuda")
        one = lambda s: None if s is None else (_dev(s, np.float32) if self.cap else torch.zeros(1, device="cuda"))
        self.smax, self.smean = one(score_max), one(score_mean)
        self.mins = _dev(np.asarray(min_score, np.float32).reshape(-1) if not torch.is_tensor(min_score) else min_score, np.float32)
        assert self.mins.numel() == self.n_cols // n_rec
        self.out_cap = self.cap if out_capacity is None else int(out_capacity)
        self.out_ptr = torch.empty(self.n_cols + 1 + TAIL, dtype=torch.int64, device="cuda")
        self.out_pairs = torch.empty(self.out_cap + TAIL, 2, dtype=torch.int32, device="cuda")
        self.omax = None if self.smax is None else torch.empty(self.out_cap + TAIL, dtype=torch.float32, device="cuda")
        self.omean = None if self.smean is None else torch.empty(self.out_cap + TAIL, dtype=torch.float32, device="cuda")
        self.err = torch.empty(2, dtype=torch.int32, device="cuda")
        self.ws_bytes = self.l.sed_events_select_ws_bytes(self.cap, self.n_cols)
        assert self.ws_bytes > 0, self.l.sed_last_error()
        self.ws = torch.empty(self.ws_bytes + TAIL, dtype=torch.uint8, device="cuda")

    def fill(self, err0=0):
        self.out_ptr.fill_(SENT)
        self.out_pairs.fill_(SENT)
        for t in (self.omax, self.omean):
            if t is not None:
                t.fill_(float(SENT))
        self.ws.fill_(0xFF)
        self.err.fill_(SENT)
        self.err[:1].fill_(err0)

    def launch(self, **kw):
        p = self._lib.ptr
        a = dict(ptr=self.ptr, pairs=self.pairs, smax=self.smax, smean=self.smean, cap=self.cap, n_cols=self.n_cols,
                 n_rec=self.n_rec, NC=self.NC, key=self.key, mins=self.mins, out_ptr=self.out_ptr, out_pairs=self.out_pairs,
                 omax=self.omax, omean=self.omean, out_cap=self.out_cap, ws=self.ws, ws_bytes=self.ws_bytes)
        a.update(kw)
        return self.l.sed_events_select(p(a["ptr"]), p(a["pairs"]), p(a["smax"]), p(a["smean"]), a["cap"], a["n_cols"], a["n_rec"],
                                        a["NC"], a["key"], p(a["mins"]), p(a["out_ptr"]), p(a["out_pairs"]), p(a["omax"]),
                                        p(a["omean"]), a["out_cap"], p(a["ws"]), a["ws_bytes"], p(self.err), self._lib.stream_ptr())

    def get(self):
        torch.cuda.synchronize()
        out_ptr, out_pairs = self.out_ptr.cpu().numpy(), self.out_pairs.cpu().numpy()
        assert (out_ptr[self.n_cols + 1:] == SENT).all() and (out_pairs[self.out_cap:] == SENT).all()
        assert int(self.err[1].item()) == SENT and (self.ws[-TAIL:] == 0xFF).all()
        scores = []
        for t in (self.omax, self.omean):
            h = None if t is None else t.cpu().numpy()
            assert h is None or (h[self.out_cap:] == SENTF).all()
            scores.append(None if h is None else h[:self.out_cap])
        return out_ptr[:self.n_cols + 1], out_pairs[:self.out_cap], scores[0], scores[1], int(self.err[0].item())

    def run(self, err0=0):
        self.fill(err0)
        assert self.launch() == 0, self.l.sed_last_error()
        return self.get()


def _table(cols, pad=5):
    """Columns (lists of (on, off)) as ev_ptr and an ev_pairs with ``pad`` sentinel rows behind the events."""
    ptr = np.r_[0, np.cumsum([len(c) for c in cols])].astype(np.int64)
    rows = [e for c in cols for e in c] + [(SENT, SENT)] * pad
    return ptr, np.asarray(rows, dtype=np.int32).reshape(-1, 2)


def _same_bits(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def _check(out, want, err=0):
    """Maxima bitwise, means within one fp32 step of the statement, NaN where it has NaN, sentinels behind the events."""
    smax, smean, e = out
    assert e == err, e
    n = len(want[0])
    _same_bits(smax[:n], want[0])
    nan = np.isnan(want[1])
    np.testing.assert_array_equal(np.isnan(smean[:n]), nan)
    diff = np.abs(smean[:n][~nan].astype(np.float64) - want[1][~nan].astype(np.float64))
    assert (diff <= np.spacing(want[1][~nan])).all(), diff.max()
    assert (smax[n:] == SENTF).all() and (smean[n:] == SENTF).all()            # nothing at or beyond ev_ptr[n_cols]


def _timeline(seed, total, NC):
    """Posteriors in [0, 1) with a spread of magnitudes (so that the order of a sum shows in its last bits)."""
    rs = np.random.RandomState(seed)
    return (rs.uniform(size=(total, NC)) ** rs.choice([1, 3, 8], size=(total, 1))).astype(np.float32)


# ---- 1. lengths, positions, shapes ---------------------------------------------------------------------------------------------
def _lengths():
    S = _short()
    return sorted({n for n in (1, 2, S - 1, S, S + 1, 63, 64, 65, 127, 128, 129, 5000) if n >= 1})


L3S = {1: [5800], 3: [700, 5800, 131]}                                         # unequal recordings


def _walk(L3, lengths, rs, from_zero, to_end):
    events, t = [], 0 if from_zero else int(rs.randint(1, 4))
    for n in np.roll(lengths, int(rs.randint(len(lengths)))):
        if t + n <= L3:
            events.append((t, t + int(n)))
            t += int(n) + int(rs.randint(1, 3))
    if to_end and t < L3:
        events.append((t, L3))
    return events


@functools.lru_cache(maxsize=None)
def _shape_case(NC, n_rec, K, variant):
    """A table over every column (k, rec, c): walks through the lengths, some from frame 0, some ending at L3, one event that
    covers its whole recording, empty columns (variant 0: in front, in the middle and behind; variant 1: column 1 only, so the
    last column holds events), and the statement's scores."""
    L3s, lengths = L3S[n_rec], _lengths()
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    n_cols = K * n_rec * NC
    empty = ({0, n_cols // 2, n_cols - 1} if n_cols >= 4 else set()) if variant == 0 else ({1} if n_cols >= 3 else set())
    whole = next((c for c in range(1, n_cols) if c not in empty), None)
    rs = np.random.RandomState(100 * NC + 10 * n_rec + K)
    cols = []
    for col in range(n_cols):
        _, rec, _ = es.column_of(col, n_rec, NC)
        cols.append([] if col in empty else [(0, L3s[rec])] if col == whole else
                    _walk(L3s[rec], lengths, rs, from_zero=col % 2 == 0, to_end=col % 3 != 1))
    ptr, pairs = _table(cols)
    tl = _timeline(NC + n_rec + K, int(f0[-1]), NC)
    tl[rs.randint(0, len(tl), size=len(tl) // 300), rs.randint(0, NC, size=len(tl) // 300)] = np.nan
    return tl, f0, ptr, pairs, es.scores(tl, f0, n_rec, NC, ptr, pairs), cols


SHAPES = [(1, 1, 1, 1, False), (3, 3, 3, 0, True), (4, 1, 3, 0, False), (4, 3, 1, 1, True), (10, 3, 1, 0, False),
          (16, 1, 1, 1, True), (16, 3, 3, 1, False), (3, 1, 1, 1, True), (10, 1, 3, 0, True)]


@pytest.mark.parametrize("NC,n_rec,K,variant,misalign", SHAPES)
def test_lengths_positions_and_shapes_against_the_statement(NC, n_rec, K, variant, misalign):
    tl, f0, ptr, pairs, want, cols = _shape_case(NC, n_rec, K, variant)
    got_lengths = {off - on for c in cols for on, off in c}
    assert got_lengths >= set(_lengths()), got_lengths
    assert any(c and c[0][0] == 0 for c in cols) and any(c and c[-1][1] in L3S[n_rec] for c in cols)
    assert variant == 0 or len(cols) == 1 or len(cols[-1]) > 0                 # events in the last column
    assert np.isnan(want[1]).any() and not np.isnan(want[0]).all()
    call = ScoresCall(tl, f0, NC, ptr, pairs, misalign)
    _check(call.run(), want)
    # one output at a time: the other buffer is not touched
    smax, smean, err = call.run(smean=None)
    assert err == 0 and (smean == SENTF).all()
    _same_bits(smax[:ptr[-1]], want[0])
    smax, smean2, err = call.run(smax=None)
    assert err == 0 and (smax == SENTF).all()
    full = call.run()
    assert smean2.tobytes() == full[1].tobytes()
    # the K-point call is K one-point calls on the slices of ev_ptr
    span = n_rec * NC
    for k in range(K):
        one = ScoresCall(tl, f0, NC, ptr[k * span:(k + 1) * span + 1], pairs, misalign).run()
        a, b = int(ptr[k * span]), int(ptr[(k + 1) * span])
        assert one[2] == 0 and one[0][a:b].tobytes() == full[0][a:b].tobytes() and one[1][a:b].tobytes() == full[1][a:b].tobytes()
        assert (np.delete(one[0], np.s_[a:b]) == SENTF).all()


# ---- 2. waves and workgroups ------------------------------------------------------------------------------------------------------
def _place(lengths_by_index, edges, L3_min=0):
    """Events of the given lengths, index by index, split into columns at ``edges``; each column packs its events with a gap
    of one frame from frame 2.  Returns the columns and the frames the longest column needs."""
    cols, need = [], 0
    for a, b in zip([0] + list(edges), list(edges) + [len(lengths_by_index)]):
        t, col = 2, []
        for n in lengths_by_index[a:b]:
            col.append((t, t + int(n)))
            t += int(n) + 1
        cols.append(col)
        need = max(need, t)
    return cols, max(need, L3_min)


def test_a_wave_with_0_1_2_and_64_long_events_in_different_columns_and_recordings():
    S = _short()
    n = np.full(4 * 64 + 70, 3)
    n[:64] = np.arange(64) % min(S, 3) + 1                                     # wave 0: no long event
    n[64:128], n[64 + 17] = 2, S + 40                                          # wave 1: one
    n[128], n[191] = S + 1, 200                                                # wave 2: its first and its last lane
    n[192:256] = S + 1 + np.arange(64) * 3                                     # wave 3: every lane, lengths on both sides of 64 and 128
    n[256:] = np.arange(70) % 5 + 1
    n[300] = 70
    cols, need = _place(n, [40, 100, 230])                                     # column edges inside the waves 0, 1 and 3
    NC, n_rec = 2, 2                                                           # columns (r0, c0) (r0, c1) (r1, c0) (r1, c1)
    L3s = [need + 3, need]
    cols[3][-1] = (cols[3][-1][0], L3s[1])                                     # the last event ends with its recording
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    tl = _timeline(5, int(f0[-1]), NC)
    ptr, pairs = _table(cols)
    want = es.scores(tl, f0, n_rec, NC, ptr, pairs)
    first = ScoresCall(tl, f0, NC, ptr, pairs).run()
    _check(first, want)
    again = ScoresCall(tl, f0, NC, ptr, pairs).run()
    assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()


@pytest.mark.parametrize("n0", [255, 256, 257])
@pytest.mark.parametrize("long_events", [False, True])
def test_events_around_a_workgroup_edge_with_the_column_edge_on_it(n0, long_events):
    S = _short()
    n = np.arange(2 * BLOCK + 9) % 4 + 1
    if long_events:
        n[253:260] = [S + 1, 64, 65, 129, 70, S + 2, 128]
    cols, need = _place(n, [n0, n0, 2 * BLOCK])                                # (an empty column on the edge as well)
    NC, f0 = 4, np.array([0, need], np.int64)
    tl = _timeline(n0, need, NC)
    ptr, pairs = _table(cols)
    _check(ScoresCall(tl, f0, NC, ptr, pairs).run(), es.scores(tl, f0, 1, NC, ptr, pairs))


def test_the_same_event_at_two_positions_has_the_same_bits():
    S = _short()
    NC, L3s = 3, [6000, 7001]
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    tl = _timeline(9, int(f0[-1]), NC)
    lengths = [1, 2, S - 1, S, S + 1, 63, 64, 65, 127, 128, 129, 5000]
    cols = [[], [], [], [], [], []]
    t_a, t_b = 3, 10
    for n in lengths:
        x = _timeline(n, n, 1)[:, 0]
        if n == 129:
            x[77] = np.nan
        tl[f0[0] + t_a:f0[0] + t_a + n, 0] = x                                # recording 0, class 0 ...
        tl[f0[1] + t_b:f0[1] + t_b + n, 2] = x                                # ... and recording 1, class 2, elsewhere in its wave
        cols[0].append((t_a, t_a + n))
        cols[5].append((t_b, t_b + n))
        t_a, t_b = t_a + n + 1, t_b + n + 2
    cols[5] = [(0, 5)] * 7 + cols[5]                                           # other lanes, another owner order
    ptr, pairs = _table(cols)
    out = ScoresCall(tl, f0, NC, ptr, pairs).run()
    _check(out, es.scores(tl, f0, 2, NC, ptr, pairs))
    a, b = slice(0, len(lengths)), slice(len(lengths) + 7, 2 * len(lengths) + 7)
    assert out[0][a].tobytes() == out[0][b].tobytes() and out[1][a].tobytes() == out[1][b].tobytes()


@functools.lru_cache(maxsize=None)
def _big_table():
    """More than 1 024 workgroups of events: two columns of one- and two-frame events, a few long ones among them."""
    rs = np.random.RandomState(2)
    n = rs.randint(1, 3, size=1024 * BLOCK + 700)
    n[[5, 70000, 140001, len(n) - 1]] = [5000, 130, 65, 300]
    cols, need = _place(n, [140000])
    NC, f0 = 2, np.array([0, need], np.int64)
    tl = _timeline(3, need, NC)
    ptr, pairs = _table(cols)
    return tl, f0, NC, ptr, pairs, es.scores(tl, f0, 1, NC, ptr, pairs)


def test_more_than_1024_workgroups_twice_and_one_graph_replay():
    tl, f0, NC, ptr, pairs, want = _big_table()
    assert ptr[-1] > 1024 * BLOCK
    call = ScoresCall(tl, f0, NC, ptr, pairs)
    eager = call.run()
    _check(eager, want)
    again = call.run()
    assert again[0].tobytes() == eager[0].tobytes() and again[1].tobytes() == eager[1].tobytes()
    graph = torch.cuda.CUDAGraph()
    call.fill()
    with torch.cuda.graph(graph):
        assert call.launch() == 0
    call.fill()
    graph.replay()
    replay = call.get()
    assert replay[2] == 0 and replay[0].tobytes() == eager[0].tobytes() and replay[1].tobytes() == eager[1].tobytes()
    # the select over the same table, twice and replayed; its compacted scores are the scores of the compacted table
    mins = np.array([[0.5, 0.7]], np.float32)
    w_sel = es.select(ptr, pairs, eager[0], eager[1], 1, NC, mins, 0)
    assert 0.1 * ptr[-1] < w_sel[0][-1] < 0.9 * ptr[-1]
    sel = SelectCall(ptr, pairs, eager[0], eager[1], 1, NC, mins)
    s_eager = sel.run()
    _check_select(s_eager, w_sel)
    graph = torch.cuda.CUDAGraph()
    sel.fill()
    with torch.cuda.graph(graph):
        assert sel.launch() == 0
    sel.fill()
    graph.replay()
    s_replay = sel.get()
    assert s_replay[4] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(s_replay[:4], s_eager[:4]))
    n = int(s_eager[0][-1])
    fresh = ScoresCall(tl, f0, NC, s_eager[0], s_eager[1][:n]).run()
    assert fresh[2] == 0 and fresh[0].tobytes() == s_eager[2][:n].tobytes() and fresh[1].tobytes() == s_eager[3][:n].tobytes()


# ---- 3. NaN frames, empty and oversized tables --------------------------------------------------------------------------------------
def test_nan_frames_inside_short_and_long_events_and_all_over_one():
    S = _short()
    NC, L3 = 3, 1200
    f0 = np.array([0, L3], np.int64)
    tl = _timeline(4, L3, NC)
    short, long_ = min(S, 5), S + 70
    cols = [[(0, short), (10, 10 + short), (20, 20 + long_), (400, 400 + long_), (800, 800 + long_), (1100, 1101)],
            [(3, 3 + short), (50, 50 + long_), (L3 - long_, L3)], []]
    tl[12, 0] = np.nan                                                         # inside a short event
    tl[[20, 20 + 64, 20 + long_ - 1], 0] = np.nan                              # inside a long one: its first, a second-stride and its last frame
    tl[800:800 + long_, 0] = np.nan                                            # a whole long event
    tl[1100, 0] = np.nan                                                       # a whole one-frame event
    tl[3:3 + short, 1] = np.nan                                                # a whole short event
    tl[L3 - long_ + 65, 1] = np.nan
    tl[:, 2] = np.nan                                                          # (class 2 has no events: never read into a score)
    ptr, pairs = _table(cols)
    want = es.scores(tl, f0, 1, NC, ptr, pairs)
    assert np.isnan(want[0]).sum() == 3 and np.isnan(want[1]).sum() == 6
    _check(ScoresCall(tl, f0, NC, ptr, pairs).run(), want)
    # a NaN score is never kept, whichever key
    out = ScoresCall(tl, f0, NC, ptr, pairs).run()
    for key in (0, 1):
        got = SelectCall(ptr, pairs, out[0], out[1], 1, NC, [[-np.inf] * NC], key).run()
        _check_select(got, es.select(ptr, pairs, out[0], out[1], 1, NC, [[-np.inf] * NC], key))
        assert got[0][-1] == ptr[-1] - (3, 6)[key]


def test_an_empty_table_and_a_capacity_far_above_the_count():
    NC, f0 = 2, np.array([0, 50], np.int64)
    tl = _timeline(6, 50, NC)
    empty = ScoresCall(tl, f0, NC, np.zeros(3, np.int64), np.zeros((0, 2), np.int32))
    assert empty.cap == 0
    assert empty.run()[2] == 0                                                 # no launch; get() checks the buffers
    sel = SelectCall(np.zeros(3, np.int64), np.zeros((0, 2), np.int32), np.zeros(0, np.float32), None, 1, NC, [[0.5] * NC]).run()
    assert sel[4] == 0 and sel[0].tolist() == [0, 0, 0]
    ptr, pairs = _table([[(0, 1), (4, 50)], []], pad=3000)                     # twelve workgroups behind two events
    out = ScoresCall(tl, f0, NC, ptr, pairs).run()
    _check(out, es.scores(tl, f0, 1, NC, ptr, pairs))
    none = ScoresCall(tl, f0, NC, np.zeros(3, np.int64), pairs).run()         # a capacity and no event
    assert none[2] == 0 and (none[0] == SENTF).all() and (none[1] == SENTF).all()
    got = SelectCall(ptr, pairs, out[0], out[1], 1, NC, [[-np.inf] * NC]).run()
    _check_select(got, (ptr, pairs[:2], out[0][:2], out[1][:2]))


# ---- 4. the error bits --------------------------------------------------------------------------------------------------------------
def _err_case():
    NC, n_rec, L3s = 2, 3, [300, 40, 500]
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    tl = _timeline(8, int(f0[-1]), NC)
    S = _short()
    cols = [[(0, 3), (5, 5 + S + 9), (200, 300)], [(1, 2)], [(0, 40)], [(2, 9), (10, 30)], [(4, 5), (100, 100 + S + 1)], [(0, 500), ]]
    return tl, f0, NC, n_rec, cols


def _column_slices(ptr):
    return [np.arange(int(ptr[c]), int(ptr[c + 1])) for c in range(len(ptr) - 1)]


@pytest.mark.parametrize("entry,value,skipped", [(0, -2, (0,)), (1, -5, (0, 1)), (6, 10 ** 6, (5,))])
def test_a_column_with_broken_bounds_raises_bit_16_and_leaves_the_other_columns_right(entry, value, skipped):
    tl, f0, NC, n_rec, cols = _err_case()
    ptr, pairs = _table(cols)
    want = es.scores(tl, f0, n_rec, NC, ptr, pairs)
    idx = _column_slices(ptr)
    bad = ptr.copy()
    bad[entry] = value
    smax, smean, err = ScoresCall(tl, f0, NC, bad, pairs).run()
    assert err == 16
    for c, ix in enumerate(idx):
        if c in skipped:
            assert (smax[ix] == SENTF).all() and (smean[ix] == SENTF).all(), c   # nothing of it is written
        else:
            _check((smax[ix], smean[ix], 0), (want[0][ix], want[1][ix]))
    out = ScoresCall(tl, f0, NC, ptr, pairs).run()
    got = SelectCall(bad, pairs, out[0], out[1], n_rec, NC, [[-np.inf] * NC]).run()
    assert got[4] == 16
    for c, ix in enumerate(idx):
        kept = got[1][got[0][c]:got[0][c + 1]]
        assert kept.tolist() == ([] if c in skipped else pairs[ix].tolist()), c


@pytest.mark.parametrize("entry,value,broken", [(1, 10 ** 6, (0, 1)), (3, 10 ** 6, (2,)), (0, -1, (0,)), (2, 290, (1, 2))])
def test_a_recording_with_broken_bounds_raises_bit_16_and_leaves_the_other_recordings_right(entry, value, broken):
    tl, f0, NC, n_rec, cols = _err_case()
    ptr, pairs = _table(cols)
    want = es.scores(tl, f0, n_rec, NC, ptr, pairs)
    bad = f0.copy()
    bad[entry] = value                                                         # 290 < f0[1]: recording 1 runs backwards, 2 stays inside
    smax, smean, err = ScoresCall(tl, bad, NC, ptr, pairs).run()
    assert err & 16 and not err & ~(16 | 64)
    for c, ix in enumerate(_column_slices(ptr)):
        rec = (c // NC) % n_rec
        a, b = int(bad[rec]), int(bad[rec + 1])
        if not 0 <= a <= b <= len(tl):
            assert (smax[ix] == SENTF).all() and (smean[ix] == SENTF).all(), c
        elif rec not in broken:
            _check((smax[ix], smean[ix], 0), (want[0][ix], want[1][ix]))


@pytest.mark.parametrize("event", [(10, 501), (7, 7), (9, 3), (-1, 4), (-5, -2), (2 ** 31 - 1, -2 ** 31)])
def test_an_event_outside_its_recording_raises_bit_64_and_scores_nan(event):
    tl, f0, NC, n_rec, cols = _err_case()
    for col, at in ((5, 0), (3, 1), (0, 1)):                                   # recordings 2, 1, 0; a short and a long neighbour
        mine = [list(c) for c in cols]
        if col != 5 and event == (10, 501):
            mine[col][at] = (10, int(f0[(col // NC) % n_rec + 1] - f0[(col // NC) % n_rec]) + 1)   # off = L3 + 1
        else:
            mine[col][at] = event
        ptr, pairs = _table(mine)
        want = es.scores(tl, f0, n_rec, NC, ptr, pairs)
        i = int(ptr[col]) + at
        assert np.isnan(want[0][i]) and np.isnan(want[1][i]) and np.isnan(want[0]).sum() == 1
        _check(ScoresCall(tl, f0, NC, ptr, pairs).run(), want, err=64)


def _check_select(got, want):
    out_ptr, out_pairs, omax, omean, err = got
    assert err == 0
    n = int(want[0][-1])
    np.testing.assert_array_equal(out_ptr, want[0])
    np.testing.assert_array_equal(out_pairs[:n], want[1])
    assert (out_pairs[n:] == SENT).all()
    for g, w in ((omax, want[2]), (omean, want[3])):
        assert (g is None) == (w is None)
        if g is not None:
            _same_bits(g[:n], w)
            assert (g[n:] == SENTF).all()


def test_the_select_with_one_event_too_many_raises_bit_2_and_writes_nothing_beyond():
    tl, f0, NC, ptr, pairs, want = _big_table()
    mins = np.array([[0.5, 0.7]], np.float32)
    w_sel = es.select(ptr, pairs, want[0], want[1], 1, NC, mins, 0)
    n = int(w_sel[0][-1])
    got = SelectCall(ptr, pairs, want[0], want[1], 1, NC, mins, out_capacity=n - 1).run()       # (get() checks the tails behind it)
    assert got[4] == 2
    np.testing.assert_array_equal(got[0], w_sel[0])                            # ALWAYS the true counts
    _check_select(SelectCall(ptr, pairs, want[0], want[1], 1, NC, mins, out_capacity=n).run(), w_sel)
    got = SelectCall(ptr, pairs, want[0], want[1], 1, NC, mins, out_capacity=0).run()
    assert got[4] == 2


def test_bad_host_arguments_return_before_any_launch():
    tl, f0, NC, n_rec, cols = _err_case()
    ptr, pairs = _table(cols)
    call = ScoresCall(tl, f0, NC, ptr, pairs)
    call.fill()
    l = call.l
    assert call.launch(tl=None) != 0 and b"null" in l.sed_last_error()
    assert call.launch(smax=None, smean=None) != 0
    assert call.launch(NC=17) != 0 and call.launch(n_cols=5) != 0 and call.launch(cap=1 << 31) != 0
    assert call.launch(total=(1 << 31) // NC) != 0
    assert call.launch(smax=call.tl) != 0 and b"overlaps" in l.sed_last_error()
    assert call.launch(smean=call.smax) != 0
    sel = SelectCall(ptr, pairs, np.zeros(len(pairs), np.float32), None, n_rec, NC, [[0.5] * NC])
    sel.fill()
    assert sel.launch(mins=None) != 0 and sel.launch(key=1) != 0 and sel.launch(out_pairs=sel.pairs) != 0
    assert sel.launch(ws_bytes=sel.ws_bytes + 8) == -2 and b"ws_bytes" in l.sed_last_error()
    torch.cuda.synchronize()
    assert (call.smax == SENT).all() and (call.smean == SENT).all() and int(call.err[0].item()) == 0
    assert (sel.out_ptr == SENT).all() and (sel.out_pairs == SENT).all() and (sel.omax == SENT).all()


# ---- 5. the select against the statement, and the cross-checks ------------------------------------------------------------------------
@pytest.mark.parametrize("NC,n_rec,K,variant", [(3, 3, 3, 0), (4, 1, 3, 0), (16, 3, 3, 1), (1, 1, 1, 1)])
def test_the_select_per_point_and_class_on_either_key(NC, n_rec, K, variant):
    tl, f0, ptr, pairs, want, _ = _shape_case(NC, n_rec, K, variant)
    smax, smean, err = ScoresCall(tl, f0, NC, ptr, pairs).run()
    rs = np.random.RandomState(K + NC)
    mins = rs.uniform(0.1, 0.9, size=(K, NC)).astype(np.float32)
    n = int(ptr[-1])
    for key in (0, 1):
        score = (smax, smean)[key][:n]
        finite = np.sort(score[~np.isnan(score)])                              # an exact tie on the key's score: dropped
        mins[0, 0] = score[0] if K * NC > 1 and not np.isnan(score[0]) else finite[len(finite) // 2]
        w = es.select(ptr, pairs, smax, smean, n_rec, NC, mins, key)
        assert n < 10 or 0 < w[0][-1] < n
        _check_select(SelectCall(ptr, pairs, smax, smean, n_rec, NC, mins, key).run(), w)
    only = SelectCall(ptr, pairs, None, smean, n_rec, NC, mins, 1).run()       # the key's array alone
    _check_select(only, es.select(ptr, pairs, None, smean, n_rec, NC, mins, 1))
    # -inf returns the table and the scores byte for byte where no score is NaN; +inf nothing
    clean = np.where(np.isnan(tl), np.float32(0.25), tl)
    smax, smean, err = ScoresCall(clean, f0, NC, ptr, pairs).run()
    got = SelectCall(ptr, pairs, smax, smean, n_rec, NC, np.full((K, NC), -np.inf, np.float32)).run()
    assert got[4] == 0 and got[0].tobytes() == ptr.tobytes() and got[1][:n].tobytes() == pairs[:n].tobytes()
    assert got[2][:n].tobytes() == smax[:n].tobytes() and got[3][:n].tobytes() == smean[:n].tobytes()
    got = SelectCall(ptr, pairs, smax, smean, n_rec, NC, np.full((K, NC), np.inf, np.float32)).run()
    assert got[4] == 0 and not got[0].any() and (got[1] == SENT).all()


@pytest.mark.parametrize("NC,hop3,weighting", HYST_GRID)
def test_decode_scores_and_select_on_the_maximum_are_the_two_threshold_decode_at_window_1(NC, hop3, weighting):
    from dcase2019_task4_amd.inference import stitch_hysteresis
    p, rec_win0, rec_frame0, tl, thr_lo, thr_hi = hysteresis_case(NC, hop3, weighting)
    K, n_rec = len(thr_lo), len(rec_frame0) - 1
    ones = np.ones((K, NC), np.int32)
    sweep = StitchCall(p, rec_win0, rec_frame0, hop3, weighting, thr_lo, ones, sweep=True)
    dec = sweep.run()
    assert dec["err"] == 0 and dec["timeline"].tobytes() == tl.tobytes()
    n_cols = K * n_rec * NC
    ev_ptr, ev_pairs = sweep.ev_ptr[:n_cols + 1], sweep.ev_pairs[:sweep.capacity]
    scores = ScoresCall(sweep.timeline, rec_frame0, NC, ev_ptr, ev_pairs)
    smax, smean, err = scores.run()
    lo_ptr, lo_pairs = decode_points(tl, rec_frame0, thr_lo, NC)
    _check((smax[:lo_ptr[-1]], smean[:lo_ptr[-1]], err), es.scores(tl, rec_frame0, n_rec, NC, lo_ptr, lo_pairs))
    sel = SelectCall(ev_ptr, ev_pairs, scores.smax[:scores.cap], scores.smean[:scores.cap], n_rec, NC, thr_hi, 0).run()
    dev = lambda a: torch.from_numpy(a).cuda()
    hyst = stitch_hysteresis(dev(p), dev(rec_win0), dev(rec_frame0), int(rec_frame0[-1]), hop3, list(thr_lo), list(thr_hi), list(ones),
                             ("uniform", "taper")[weighting])
    h_ptr = hyst["ev_ptr"].cpu().numpy()
    n = int(h_ptr[-1])
    assert int(hyst["err"].item()) == 0 and sel[4] == 0 and 0 < n < lo_ptr[-1]
    assert sel[0].tobytes() == h_ptr.tobytes() and sel[1][:n].tobytes() == hyst["ev_pairs"].cpu().numpy()[:n].tobytes()
    # the compacted scores are the scores of the compacted table, computed afresh
    fresh = ScoresCall(sweep.timeline, rec_frame0, NC, sel[0], sel[1][:n]).run()
    assert fresh[2] == 0 and fresh[0].tobytes() == sel[2][:n].tobytes() and fresh[1].tobytes() == sel[3][:n].tobytes()


def test_a_batch_of_clips_is_one_window_recordings():
    from dcase2019_task4_amd.inference import events_scores, events_select, postprocess
    n, T, NC = 5, 157, 4
    strong = np.stack([smooth_timeline(70 + i, T, NC) for i in range(n)])
    d_strong = torch.from_numpy(strong).cuda()
    cnt, pairs = postprocess(d_strong, 0.5, 3)
    cnt, pairs = cnt.cpu().numpy(), pairs.cpu().numpy()
    cols = [[tuple(int(v) for v in e) for e in pairs[i, c, :cnt[i, c]]] for i in range(n) for c in range(NC)]
    ptr, flat = _table(cols, pad=2)
    assert ptr[-1] > 20
    f0 = np.arange(n + 1, dtype=np.int64) * T
    want = es.scores(strong.reshape(n * T, NC), f0, n, NC, ptr, flat)
    d_ptr, d_pairs, d_f0 = torch.from_numpy(ptr).cuda(), torch.from_numpy(flat).cuda(), torch.from_numpy(f0).cuda()
    smax, smean, err = events_scores((d_ptr, d_pairs), d_strong.reshape(n * T, NC), d_f0, n, NC)
    m = int(ptr[-1])
    _check((np.r_[smax.cpu().numpy()[:m]], np.r_[smean.cpu().numpy()[:m]], int(err.item())), want)
    # the Python fronts: one score only, a given error word, scalar / per-class / [K, NC] / device minima
    only_max, none, word = events_scores({"ev_ptr": d_ptr, "ev_pairs": d_pairs}, d_strong.reshape(n * T, NC), d_f0, n, NC, want="max",
                                         err=torch.full((1,), 8, dtype=torch.int32, device="cuda"))
    assert none is None and int(word.item()) == 8 and torch.equal(only_max[:m], smax[:m])
    w = es.select(ptr, flat, want[0], want[1], n, NC, [[0.8] * NC], 0)
    assert 0 < w[0][-1] < m
    for mins in (0.8, [0.8] * NC, np.full((1, NC), 0.8, np.float32), torch.full((NC,), 0.8, device="cuda")):
        out = events_select(d_ptr, d_pairs, smax, smean, n, NC, mins)
        assert int(out[4].item()) == 0 and out[1].shape[0] == flat.shape[0]
        np.testing.assert_array_equal(out[0].cpu().numpy(), w[0])
        np.testing.assert_array_equal(out[1].cpu().numpy()[:w[0][-1]], w[1])
        _same_bits(out[2].cpu().numpy()[:w[0][-1]], w[2])
    word = torch.full((1,), 8, dtype=torch.int32, device="cuda")
    out = events_select(d_ptr, d_pairs, None, smean, n, NC, 0.0, key="mean", capacity=1, err=word)
    assert out[4] is word and int(word.item()) == 8 | 2 and out[2] is None and out[3].shape[0] == 1
    with pytest.raises(ValueError):
        events_select(d_ptr, d_pairs, smax, None, n, NC, 0.6, key="mean")
    with pytest.raises(ValueError):
        events_select(d_ptr, d_pairs, smax, smean, n, NC, [0.5, 0.6])
    with pytest.raises(ValueError):
        events_scores((d_ptr, d_pairs), d_strong.reshape(n * T, NC), d_f0, n + 1, NC)


def test_score_decoded_and_select_decoded_on_a_stitch_dict():
    from dcase2019_task4_amd.inference import score_decoded, select_decoded, stitch_decode, stitch_sweep
    NC, hop3, weighting = 3, 8, 1
    p, rec_win0, rec_frame0, tl, thr_lo, thr_hi = hysteresis_case(NC, hop3, weighting)
    n_rec = len(rec_frame0) - 1
    dev = lambda a: torch.from_numpy(a).cuda()
    d_f0 = dev(rec_frame0)
    out = stitch_sweep(dev(p), dev(rec_win0), d_f0, int(rec_frame0[-1]), hop3, list(thr_lo), [3], want_timeline=True)
    scored = score_decoded(out, d_f0, n_rec, NC)
    assert scored["err"] is out["err"] and int(scored["err"].item()) == 0 and scored["ev_ptr"] is out["ev_ptr"]
    ptr, pairs = out["ev_ptr"].cpu().numpy(), out["ev_pairs"].cpu().numpy()
    n = int(ptr[-1])
    want = es.scores(tl, rec_frame0, n_rec, NC, ptr, pairs[:n])
    _check((scored["score_max"].cpu().numpy()[:n], scored["score_mean"].cpu().numpy()[:n], 0), want)
    w = es.select(ptr, pairs, want[0], scored["score_mean"].cpu().numpy(), n_rec, NC, thr_hi, 1)
    for d in (select_decoded(scored, d_f0, n_rec, NC, thr_hi, key="mean"), select_decoded(out, d_f0, n_rec, NC, thr_hi, key="mean")):
        assert int(d["err"].item()) == 0 and d["n_points"] == len(thr_lo) and d["timeline"] is out["timeline"]
        np.testing.assert_array_equal(d["ev_ptr"].cpu().numpy(), w[0])
        np.testing.assert_array_equal(d["ev_pairs"].cpu().numpy()[:w[0][-1]], w[1])
        _same_bits(d["score_mean"].cpu().numpy()[:w[0][-1]], w[3])
    assert 0 < w[0][-1] < n
    plain = stitch_decode(dev(p), dev(rec_win0), d_f0, int(rec_frame0[-1]), hop3, thr_lo[0], 3, want_timeline=False)
    with pytest.raises(ValueError, match="timeline"):
        score_decoded(plain, d_f0, n_rec, NC)
    with pytest.raises(ValueError, match="timeline"):
        select_decoded(plain, d_f0, n_rec, NC, 0.5)


# ---- 6. get_long_predictions ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_case():
    from dcase2019_task4_amd.inference import LongRecordingSet, get_long_predictions
    labels = [f"c{i}" for i in range(10)]
    model, _ = gu.make_model(0)
    model.eval()
    rs = np.random.RandomState(21)
    feats = [(np.abs(rs.standard_normal((L, 64))) ** 2 * np.exp(rs.uniform(-6, 2, (L, 1))) + 1e-6).astype(np.float32)
             for L in (40, 64, 900)]
    names = ["a.wav", "b.wav", "c.wav"]
    lset = LongRecordingSet.from_arrays(feats, 64, scaler=_Scaler(64), filenames=names)
    plain, timelines, _ = get_long_predictions(model, lset, labels, batch_size=8, return_posteriors=True)
    tl = torch.cat(timelines).cpu().numpy()
    thr = np.quantile(tl, 0.5, axis=0).astype(np.float32)
    return model, lset, labels, names, tl, thr


def _statement_columns(df, tl, f0, names, labels):
    """score_max / score_mean of the rows of ``df`` by the statement, from the frames its seconds stand for."""
    smax, smean = [], []
    for row in df.itertuples(index=False):
        on, off = int(round(row.onset * DEN / NUM)), int(round(row.offset * DEN / NUM))
        assert on * NUM / DEN == row.onset and off * NUM / DEN == row.offset
        base, c = int(f0[names.index(row.filename)]), labels.index(row.event_label)
        values = [tl[base + u, c] for u in range(on, off)]
        smax.append(es.event_max(values))
        smean.append(es.event_mean(values))
    return np.asarray(smax, np.float32), np.asarray(smean, np.float32)


def test_get_long_predictions_defaults_are_unchanged_and_reach_no_new_entry(monkeypatch):
    from dcase2019_task4_amd import inference
    model, lset, labels, names, tl, thr = _long_case()
    kw = dict(batch_size=8, threshold=thr, median_window=3)
    before = inference.get_long_predictions(model, lset, labels, **kw)
    spelled = inference.get_long_predictions(model, lset, labels, event_scores=False, min_event_score=None, score_key="max", **kw)
    assert list(before.columns) == ["event_label", "onset", "offset", "filename"] == list(spelled.columns)
    assert before.equals(spelled) and (before.index == spelled.index).all() and len(before) > 30

    def never(*a, **k):
        raise AssertionError("a new entry point was reached with the defaults")
    monkeypatch.setattr(inference, "events_scores", never)
    monkeypatch.setattr(inference, "events_select", never)
    l = inference._lib.lib()
    for name in ("sed_events_scores", "sed_events_select"):
        monkeypatch.setattr(l, name, never, raising=False)
    again = inference.get_long_predictions(model, lset, labels, threshold_high=np.quantile(tl, 0.8, axis=0).astype(np.float32),
                                           min_event_length=0.2, **kw)
    assert list(again.columns) == list(before.columns) and 0 < len(again) < len(before)
    assert inference.get_long_predictions(model, lset, labels, **kw).equals(before)


def test_get_long_predictions_with_scores_and_a_minimum_score(tmp_path):
    from dcase2019_task4_amd.inference import get_long_predictions
    model, lset, labels, names, tl, thr = _long_case()
    f0 = lset.rec_frame0_host
    kw = dict(batch_size=8, threshold=thr, median_window=3)
    plain = get_long_predictions(model, lset, labels, **kw)
    path = str(tmp_path / "scored.tsv")
    df, timelines, _ = get_long_predictions(model, lset, labels, event_scores=True, return_posteriors=True, save_predictions=path, **kw)
    assert list(df.columns) == ["event_label", "onset", "offset", "filename", "score_max", "score_mean"]
    assert df[list(plain.columns)].equals(plain) and df.score_max.dtype == np.float32
    assert torch.cat(timelines).cpu().numpy().tobytes() == tl.tobytes()
    want = _statement_columns(df, tl, f0, names, labels)
    _check((df.score_max.to_numpy(), df.score_mean.to_numpy(), 0), want)
    assert open(path).readline().rstrip("\n").split("\t") == list(df.columns)
    alone = get_long_predictions(model, lset, labels, event_scores=True, **kw)                    # without return_posteriors
    assert alone.equals(df)
    # a minimum score: the rows the statement keeps, scalar or per class, on either key
    for key, column in (("max", "score_max"), ("mean", "score_mean")):
        m = np.quantile(df[column].to_numpy(), 0.6).astype(np.float32)
        per_class = (m * np.linspace(0.9, 1.1, len(labels))).astype(np.float32)
        for mins, keep in ((float(m), df[column].to_numpy() > m),
                           (per_class, df[column].to_numpy() > per_class[[labels.index(e) for e in df.event_label]])):
            sel = get_long_predictions(model, lset, labels, min_event_score=mins, score_key=key, **kw)
            assert 0 < keep.sum() < len(df) and list(sel.columns) == list(df.columns)
            assert sel.reset_index(drop=True).equals(df[keep].reset_index(drop=True))
    # together with a high threshold and a minimum length: the scores of the final table, then the select
    high = np.quantile(tl, 0.8, axis=0).astype(np.float32)
    extra = dict(threshold_high=high, min_event_length=0.3, min_event_gap=0.2, **kw)
    base = get_long_predictions(model, lset, labels, **extra)
    scored = get_long_predictions(model, lset, labels, event_scores=True, **extra)
    assert scored[list(base.columns)].equals(base) and 0 < len(base) < len(plain)
    want = _statement_columns(scored, tl, f0, names, labels)                   # fused events: their whole span, gaps included
    _check((scored.score_max.to_numpy(), scored.score_mean.to_numpy(), 0), want)
    m = float(np.median(scored.score_mean.to_numpy()))
    sel = get_long_predictions(model, lset, labels, min_event_score=m, score_key="mean", **extra)
    keep = scored.score_mean.to_numpy() > np.float32(m)
    assert 0 < keep.sum() < len(scored) and sel.reset_index(drop=True).equals(scored[keep].reset_index(drop=True))


def test_get_long_predictions_refuses_bad_score_arguments_before_any_forward(monkeypatch):
    from dcase2019_task4_amd import inference
    model, lset, labels, names, tl, thr = _long_case()

    def never(*a, **k):
        raise AssertionError("a forward ran before the arguments were checked")
    monkeypatch.setattr(inference, "long_window_posteriors", never)
    for kw in (dict(score_key="median"), dict(min_event_score=[0.1, 0.2]), dict(min_event_score=float("nan")),
               dict(event_scores="yes"), dict(event_scores=True, score_key=0)):
        with pytest.raises(ValueError):
            inference.get_long_predictions(model, lset, labels, **kw)

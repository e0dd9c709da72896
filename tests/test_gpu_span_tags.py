"""-m gpu tests of the span-level weak tags and the tag gate against the plain-loop statement (tests/span_tags_np.py):
sed_stitch_span_tags (shapes, span lengths around the tile, bit-identity with sed_stitch_weak at one span per recording, equal
spans = equal bits, error bits, bad arguments, two calls and a graph replay), sed_events_tag_scores and the gate built from it
and sed_events_select (spans touched on both sides of the thread / wave boundary, span boundaries, waves and workgroups, NaN
tags, the error bits, -inf, K points = K calls, graph replay), and get_long_predictions / validate_long end to end on the small
model of tests/test_gpu_long_weak.py.  Every buffer a kernel writes starts as NaN / sentinel bytes and carries a tail that
must come back untouched.

Bounds (derived, not measured): a span's fp64 sums are any-order sums of len non-negative terms, so they lie within
(len - 1) * 2^-53 relative of the exactly rounded (math.fsum) values; the tag is one fp64 division and one rounding to fp32
away: within one fp32 step of the statement's.  Tag scores are copies of input values: compared bitwise."""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from tests import event_scores_np as es
from tests import gpu_util as gu
from tests import span_tags_np as sp
from tests import stitch_np, weak_np
from tests.long_util import SENT, TAIL, _Scaler, _tables, _tile
from tests.test_gpu_event_scores import SENTF, SelectCall, _same_bits, _short, _table
from tests.test_gpu_long import FRAMES, LABELS, _recordings
from tests.test_gpu_long_weak import U64, WeakCall, _ulps

pytestmark = pytest.mark.gpu

BLOCK = 256


class SpanCall(WeakCall):
    """One sed_stitch_span_tags call on sentinel-filled outputs, as WeakCall: NaN tags / sums with a tail of TAIL NaNs, a 0xFF
    workspace with a tail, a second error word.  ``rec_span0``: the table given to the call (default: the right one)."""

    def __init__(self, p, a, rec_win0, rec_frame0, hop3, weighting, span3, misalign=None, rec_span0=None, total_spans=None):
        super().__init__(p, a, rec_win0, rec_frame0, hop3, weighting, misalign)
        self.span3 = int(span3)
        self.span0_host = sp.span_table(np.diff(np.asarray(rec_frame0, np.int64)), self.span3) if rec_span0 is None \
            else np.asarray(rec_span0, np.int64)
        self.total_spans = int(self.span0_host[-1]) if total_spans is None else int(total_spans)
        self.rec_span0 = torch.from_numpy(self.span0_host).cuda()
        n = self.total_spans * self.NC
        self.weak = torch.empty(n + TAIL, dtype=torch.float32, device="cuda")
        self.sums = torch.empty(2 * n + TAIL, dtype=torch.float64, device="cuda")
        self.ws_bytes = self.l.sed_stitch_span_tags_ws_bytes(self.total, self.total_spans, self.n_rec, self.NC, self.span3)
        assert self.ws_bytes > 0, self.l.sed_last_error()
        self.ws = torch.empty(self.ws_bytes + TAIL, dtype=torch.uint8, device="cuda")

    def launch(self, **kw):
        ptr = self._lib.ptr
        a = dict(p=self.p, a=self.a, span0=self.rec_span0, total=self.total, total_spans=self.total_spans, n_rec=self.n_rec,
                 T3=self.T3, NC=self.NC, hop3=self.hop3, weighting=self.weighting, span3=self.span3, weak=self.weak,
                 sums=self.sums, ws=self.ws, ws_bytes=self.ws_bytes)
        a.update(kw)
        return self.l.sed_stitch_span_tags(ptr(a["p"]), ptr(a["a"]), ptr(self.rec_win0), ptr(self.rec_frame0), ptr(a["span0"]),
                                           a["total"], a["total_spans"], a["n_rec"], a["T3"], a["NC"], a["hop3"], a["weighting"],
                                           a["span3"], ptr(a["weak"]), ptr(a["sums"]), ptr(a["ws"]), a["ws_bytes"], ptr(self.err),
                                           self._lib.stream_ptr())

    def get(self):
        torch.cuda.synchronize()
        n = self.total_spans * self.NC
        tags, sums = self.weak.cpu().numpy(), self.sums.cpu().numpy()
        assert np.isnan(tags[n:]).all() and np.isnan(sums[2 * n:]).all()
        assert int(self.err[1].item()) == SENT and (self.ws[-TAIL:] == 0xFF).all()
        return {"tags": tags[:n].reshape(self.total_spans, self.NC), "sums": sums[:2 * n].reshape(self.total_spans, self.NC, 2),
                "err": int(self.err[0].item())}


def _inputs(rs, n_win, T3, NC):
    return rs.uniform(size=(n_win, T3, NC)).astype(np.float32), weak_np.attention(rs, n_win, T3, NC)


def _span_lengths(L3s, span3):
    return [min(span3, L - s * span3) for L in L3s for s in range(-(-L // span3))]


def _check(got, want_tags, want_sums, lens, what):
    """The two bounds of the module docstring, span by span; prints how many tags are not bit-equal to the statement."""
    assert got["tags"].shape == want_tags.shape
    n_diff = 0
    for g, n in enumerate(lens):
        bound = (n - 1) * U64 * want_sums[g]
        assert (np.abs(got["sums"][g] - want_sums[g]) <= bound).all(), (what, g, got["sums"][g], want_sums[g])
        d = _ulps(got["tags"][g], want_tags[g])
        assert (d <= 1).all(), (what, g, got["tags"][g], want_tags[g])
        n_diff += int((d != 0).sum())
    print(f"{what}: {n_diff} of {want_tags.size} tags not bit-equal to the statement")


_BLEND = {}


def _blended(p, a, rec_win0, rec_frame0, hop3, weighting):
    """The statement's two blends, computed once per input (the misaligned cases share the aligned case's inputs)."""
    key = (p.tobytes(), a.tobytes(), tuple(rec_win0), tuple(rec_frame0), hop3, weighting)
    if key not in _BLEND:
        _BLEND.clear()
        _BLEND[key] = (stitch_np.blend(p, rec_win0, rec_frame0, hop3, weighting), stitch_np.blend(a, rec_win0, rec_frame0, hop3, weighting))
    return _BLEND[key]


def _span3s(t):
    return [1, 3, 8, t - 1, t, t + 1, 2 * t + 6]


# ---- 1. the span tags against the statement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", [1, 3, 8])
@pytest.mark.parametrize("NC,misalign", [(1, None), (3, None), (10, None), (12, None), (12, "p"), (12, "a")])
def test_tags_and_sums_match_the_fsum_statement(NC, misalign, hop3, weighting):
    """Scalar path (NC = 1, 3, 10; NC = 12 with either input off 16-byte alignment) and 16-byte path (NC = 12); every length
    around the window and the tile as recordings of ONE call; spans of one frame, with a short last span, of exactly one tile,
    of two tiles plus a remainder, and one span per recording."""
    T3, t = 8, _tile()
    L3s = [1, 7, 8, 9, 8 + hop3, t - 1, t, t + 1, 2 * t + 5]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    rs = np.random.RandomState(1000 + 100 * NC + 10 * hop3 + weighting)
    p, a = _inputs(rs, rec_win0[-1], T3, NC)
    P, A = _blended(p, a, rec_win0, rec_frame0, hop3, weighting)
    for span3 in _span3s(t):
        got = SpanCall(p, a, rec_win0, rec_frame0, hop3, weighting, span3, misalign=misalign).run()
        assert got["err"] == 0
        want_tags, want_sums, rec_span0 = sp.pool_timelines(P, A, rec_frame0, span3)
        assert got["tags"].shape[0] == rec_span0[-1]
        _check(got, want_tags, want_sums, _span_lengths(L3s, span3),
               f"NC={NC} misalign={misalign} hop3={hop3} weighting={weighting} span3={span3}")
        if misalign is not None:                   # the summation order does not depend on the path: identical bytes
            aligned = SpanCall(p, a, rec_win0, rec_frame0, hop3, weighting, span3).run()
            assert aligned["tags"].tobytes() == got["tags"].tobytes() and aligned["sums"].tobytes() == got["sums"].tobytes()


@pytest.mark.parametrize("NC,hop3,misalign", [(3, 3, None), (12, 1, None), (12, 8, "a"), (10, 8, None)])
def test_one_span_per_recording_is_sed_stitch_weak_bit_for_bit(NC, hop3, misalign):
    T3, t = 8, _tile()
    L3s = [1, 7, 8, 9, t - 1, t, t + 1, 2 * t + 5, 3 * t + 1]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    p, a = _inputs(np.random.RandomState(40 + NC + hop3), rec_win0[-1], T3, NC)
    weak = WeakCall(p, a, rec_win0, rec_frame0, hop3, 1, misalign=misalign).run()
    for span3 in (max(L3s), max(L3s) + 7, 10 * max(L3s)):
        got = SpanCall(p, a, rec_win0, rec_frame0, hop3, 1, span3, misalign=misalign).run()
        assert got["err"] == 0 and weak["err"] == 0 and got["tags"].shape == (len(L3s), NC)
        assert got["tags"].tobytes() == weak["weak"].tobytes() and got["sums"].tobytes() == weak["sums"].tobytes()


@pytest.mark.parametrize("NC", [3, 12])
@pytest.mark.parametrize("n_w", [1, 3, 64, 65, 130])
def test_equal_spans_give_equal_bits_wherever_they_lie(NC, n_w):
    """hop3 == T3 (every frame is one window's, copied exactly) and a window tensor that repeats with the span's period: the
    spans of n_w windows all hold the same frames - at three positions in recording 0 (tile-relative offsets differ as soon as
    a span is no multiple of the tile) and at the head of recording 1, whose last span is shorter."""
    T3 = 8
    span3 = n_w * T3
    base_p, base_a = _inputs(np.random.RandomState(7 * NC + n_w), n_w, T3, NC)
    L3s = [3 * span3, span3 + 5]
    rec_win0, rec_frame0 = _tables(L3s, T3, T3)
    reps = -(-int(rec_win0[-1]) // n_w)
    p, a = np.tile(base_p, (reps, 1, 1))[:rec_win0[-1]], np.tile(base_a, (reps, 1, 1))[:rec_win0[-1]]
    got = SpanCall(p, a, rec_win0, rec_frame0, T3, 1, span3).run()
    assert got["err"] == 0 and got["tags"].shape[0] == 5
    for g in (1, 2, 3):
        assert got["tags"][g].tobytes() == got["tags"][0].tobytes() and got["sums"][g].tobytes() == got["sums"][0].tobytes()
    assert got["sums"][4].tobytes() != got["sums"][0].tobytes()
    # ... and they are the bits sed_stitch_weak gives a recording of that length
    w0, f0 = _tables([span3], T3, T3)
    weak = WeakCall(base_p, base_a, w0, f0, T3, 1).run()
    assert weak["weak"].tobytes() == got["tags"][0].tobytes() and weak["sums"].tobytes() == got["sums"][0].tobytes()


def test_two_calls_and_a_graph_replay_give_identical_bytes():
    T3, NC, hop3 = 8, 10, 3
    L3s = [3 * _tile() + 9, 5, 40]
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    p, a = _inputs(np.random.RandomState(74), rec_win0[-1], T3, NC)
    call = SpanCall(p, a, rec_win0, rec_frame0, hop3, 1, _tile() + 3)
    first = call.run()
    second = call.run()
    assert first["err"] == 0 and not np.isnan(first["tags"]).any()
    graph = torch.cuda.CUDAGraph()
    call.fill()
    with torch.cuda.graph(graph):
        assert call.launch() == 0
    call.fill()
    graph.replay()
    third = call.get()
    for other in (second, third):
        assert other["err"] == 0
        assert first["tags"].tobytes() == other["tags"].tobytes() and first["sums"].tobytes() == other["sums"].tobytes()


# ---- 2. error bits and bad arguments ------------------------------------------------------------------------------------------
def _err_case():
    T3, NC, hop3, span3 = 8, 3, 4, 5
    L3s = [12, 5, 23, 9, 30]                                                     # 3, 1, 5, 2, 6 spans
    rec_win0, rec_frame0 = _tables(L3s, T3, hop3)
    p, a = _inputs(np.random.RandomState(80), rec_win0[-1], T3, NC)
    return T3, NC, hop3, span3, L3s, rec_win0, rec_frame0, p, a


def _check_rows(got, clean, table, good_table, bad_recs, n_rec):
    """Every row that no valid recording holds by the GIVEN table is NaN - never stale -, and the rows of every recording
    outside ``bad_recs`` equal the clean call's, byte for byte."""
    rows = np.zeros(got["tags"].shape[0], bool)
    for r in set(range(n_rec)) - set(bad_recs):
        a, b, c, d = int(table[r]), int(table[r + 1]), int(good_table[r]), int(good_table[r + 1])
        rows[a:b] = True
        assert got["tags"][a:b].tobytes() == clean["tags"][c:d].tobytes(), r
        assert got["sums"][a:b].tobytes() == clean["sums"][c:d].tobytes(), r
    assert np.isnan(got["tags"][~rows]).all() and np.isnan(got["sums"][~rows]).all() and not np.isnan(got["tags"][rows]).any()
    assert (~rows).any()


@pytest.mark.parametrize("case", ["one_span_fewer", "one_span_more", "not_increasing", "other_span3"])
def test_a_rec_span0_that_disagrees_raises_bit_16_and_only_those_rows_are_nan(case):
    T3, NC, hop3, span3, L3s, rec_win0, rec_frame0, p, a = _err_case()
    clean = SpanCall(p, a, rec_win0, rec_frame0, hop3, 1, span3).run()
    good = sp.span_table(L3s, span3)
    assert clean["err"] == 0 and good.tolist() == [0, 3, 4, 9, 11, 17]
    if case == "one_span_fewer":                                                 # recording 2 one short, recording 3 one over
        table, bad = good.copy(), {2, 3}
        table[3] -= 1
    elif case == "one_span_more":                                                # recording 2 is given six spans, the rest shifts
        table, bad = good.copy(), {2}
        table[3:] += 1
    elif case == "not_increasing":                                               # recording 3 runs backwards, recording 4 is too long
        table, bad = good.copy(), {3, 4}
        table[4] = 8
    else:                                                                        # the table of span3 = 6: 2, 1, 4, 2, 5 spans
        table = sp.span_table(L3s, 6)
        bad = {r for r in range(5) if table[r + 1] - table[r] != good[r + 1] - good[r]}
        assert bad == {0, 2, 4}
    got = SpanCall(p, a, rec_win0, rec_frame0, hop3, 1, span3, rec_span0=table).run()       # (get() checks the tails)
    assert got["err"] == 16
    _check_rows(got, clean, table, good, bad, len(L3s))


def test_a_total_below_the_table_raises_bit_16():
    """rec_span0 reaches beyond total_spans: the recordings that do are refused, nothing is written beyond the outputs."""
    T3, NC, hop3, span3, L3s, rec_win0, rec_frame0, p, a = _err_case()
    clean = SpanCall(p, a, rec_win0, rec_frame0, hop3, 1, span3).run()
    good = sp.span_table(L3s, span3)
    got = SpanCall(p, a, rec_win0, rec_frame0, hop3, 1, span3, rec_span0=good, total_spans=12).run()
    assert got["err"] == 16 and got["tags"].shape[0] == 12
    _check_rows(got, clean, good, good, {4}, len(L3s))


def test_too_few_windows_raise_bit_32_and_only_those_rows_are_nan():
    """Recording 1 needs 4 windows and is given 2."""
    T3, NC, span3 = 8, 3, 5
    p, a = _inputs(np.random.RandomState(70), 4, T3, NC)
    rec_win0, rec_frame0 = [0, 1, 3, 4], [0, 8, 38, 46]
    got = SpanCall(p, a, rec_win0, rec_frame0, T3, 0, span3).run()
    assert got["err"] == 32 and got["tags"].shape[0] == 2 + 6 + 2
    assert np.isnan(got["tags"][2:8]).all() and np.isnan(got["sums"][2:8]).all()
    for r, (w0, rows) in {0: (0, slice(0, 2)), 2: (3, slice(8, 10))}.items():
        want_tags, want_sums, _ = sp.pool(p[w0:w0 + 1], a[w0:w0 + 1], [0, 1], [0, 8], T3, 0, span3)
        _check({"tags": got["tags"][rows], "sums": got["sums"][rows]}, want_tags, want_sums, [5, 3], f"row {r}")


def test_bad_host_arguments_return_before_any_launch():
    T3, NC, hop3, span3, L3s, rec_win0, rec_frame0, p, a = _err_case()
    call = SpanCall(p, a, rec_win0, rec_frame0, hop3, 0, span3)
    call.fill()
    for kw in (dict(NC=17), dict(NC=0), dict(hop3=0), dict(hop3=9), dict(T3=0), dict(T3=4097, hop3=1), dict(weighting=2),
               dict(n_rec=0), dict(p=None), dict(a=None), dict(weak=None), dict(ws=None), dict(span0=None), dict(span3=0),
               dict(span3=-4), dict(total_spans=0), dict(total_spans=4), dict(total_spans=call.total + 1), dict(total=0),
               dict(total=(1 << 31) // NC + 1), dict(ws_bytes=call.ws_bytes + 8), dict(ws_bytes=call.ws_bytes - NC * 16),
               dict(ws_bytes=0), dict(span3=_tile() + 1), dict(total_spans=call.total_spans + 1)):
        assert call.launch(**kw) == -1, kw                                       # SED_ERR_BAD_ARG (the last two: ws_bytes is another call's)
    assert call.untouched()
    l, t = call.l, _tile()
    fn = l.sed_stitch_span_tags_ws_bytes
    assert fn(100, 10, 2, 10, 0) == 0 and fn(100, 10, 2, 17, 8) == 0 and fn(100, 1, 2, 10, 8) == 0 and fn(100, 101, 2, 10, 8) == 0
    assert fn(1 << 28, 10, 2, 10, 8) == 0 and fn(0, 0, 1, 10, 8) == 0
    assert fn(1 << 26, 1 << 26, 1, 1, t + 1) > 0 and fn(1 << 26, 1 << 26, 1, 1, 32 * t + 1) == 0      # tile slots < 2^31
    assert fn(100, 10, 2, 10, 8) == 10 * 10 * 16 and fn(5000, 7, 2, 3, 2 * t + 1) == 7 * 3 * 3 * 16
    assert call.launch(sums=None) == 0                                            # sums is optional
    got = call.get()
    assert got["err"] == 0 and np.isnan(got["sums"]).all() and not np.isnan(got["tags"]).any()


# ---- 3. tag scores and the gate -------------------------------------------------------------------------------------------------
def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


class TagCall:
    """One sed_events_tag_scores call on a sentinel-filled output with a tail of TAIL elements that ``get()`` checks."""

    def __init__(self, tags, rec_span0, span3, NC, ev_ptr, ev_pairs):
        from dcase2019_task4_amd import _lib
        self._lib, self.l, self.NC, self.span3 = _lib, _lib.lib(), NC, int(span3)
        self.tags = _dev(np.asarray(tags, np.float32).reshape(-1), np.float32)
        self.total_spans = self.tags.numel() // NC
        self.s0, self.ptr = _dev(rec_span0, np.int64), _dev(ev_ptr, np.int64)
        self.pairs = _dev(np.asarray(ev_pairs).reshape(-1, 2), np.int32)
        self.n_rec, self.n_cols, self.cap = self.s0.numel() - 1, self.ptr.numel() - 1, self.pairs.shape[0]
        self.score = torch.empty(self.cap + TAIL, dtype=torch.float32, device="cuda")
        self.err = torch.empty(2, dtype=torch.int32, device="cuda")

    def fill(self):
        self.score.fill_(float(SENT))
        self.err.fill_(SENT)
        self.err[:1].zero_()

    def launch(self, **kw):
        p = self._lib.ptr
        a = dict(tags=self.tags, total_spans=self.total_spans, s0=self.s0, span3=self.span3, n_rec=self.n_rec, NC=self.NC,
                 ptr=self.ptr, pairs=self.pairs, cap=self.cap, n_cols=self.n_cols, score=self.score)
        a.update(kw)
        return self.l.sed_events_tag_scores(p(a["tags"]), a["total_spans"], p(a["s0"]), a["span3"], a["n_rec"], a["NC"],
                                            p(a["ptr"]), p(a["pairs"]), a["cap"], a["n_cols"], p(a["score"]), p(self.err),
                                            self._lib.stream_ptr())

    def get(self):
        torch.cuda.synchronize()
        score = self.score.cpu().numpy()
        assert (score[self.cap:] == SENTF).all() and int(self.err[1].item()) == SENT
        return score[:self.cap], int(self.err[0].item())

    def run(self, **kw):
        self.fill()
        assert self.launch(**kw) == 0, self.l.sed_last_error()
        return self.get()


def _check_scores(out, want, err=0):
    score, e = out
    assert e == err, e
    n = len(want)
    _same_bits(score[:n], want)
    assert (score[n:] == SENTF).all()                                            # nothing at or beyond ev_ptr[n_cols]


def _check_gate(got, want):
    out_ptr, out_pairs, kept, _, err = got
    assert err == 0
    n = int(want[0][-1])
    np.testing.assert_array_equal(out_ptr, want[0])
    np.testing.assert_array_equal(out_pairs[:n], want[1])
    assert (out_pairs[n:] == SENT).all() and (kept[n:] == SENTF).all()
    _same_bits(kept[:n], want[2])


def _tags(seed, total_spans, NC, nan_every=0):
    rs = np.random.RandomState(seed)
    tags = rs.uniform(size=(total_spans, NC)).astype(np.float32)
    if nan_every:
        tags[rs.randint(0, total_spans, size=max(total_spans // nan_every, 1)), rs.randint(0, NC, size=max(total_spans // nan_every, 1))] = np.nan
    return tags


def _random_columns(rs, L3s, n_rec, NC, K, max_len):
    cols = []
    for col in range(K * n_rec * NC):
        _, rec, _ = es.column_of(col, n_rec, NC)
        t, col_events = int(rs.randint(0, 3)), []
        while rs.uniform() < 0.93:
            n = int(rs.randint(1, max_len))
            if t + n > L3s[rec]:
                break
            col_events.append((t, t + n))
            t += n + int(rs.randint(1, 4))
        cols.append(col_events if col % 7 != 3 else [])
    return cols


@pytest.mark.parametrize("NC,n_rec,K,span3", [(1, 1, 1, 1), (3, 3, 3, 4), (4, 1, 3, 7), (10, 3, 1, 3), (16, 3, 2, 50)])
def test_random_tables_over_random_tags_and_the_gate_against_the_statement(NC, n_rec, K, span3):
    rs = np.random.RandomState(100 * NC + 10 * n_rec + K)
    L3s = [700, 5800, 131][:n_rec] if n_rec > 1 else [5800]
    rec_span0 = sp.span_table(L3s, span3)
    tags = _tags(NC + K, int(rec_span0[-1]), NC, nan_every=40)
    cols = _random_columns(rs, L3s, n_rec, NC, K, 400)
    cols[-1] = cols[-1] + [(L3s[-1] - 1, L3s[-1])]                               # an event in the (short) last span
    ptr, pairs = _table(cols)
    want = sp.tag_scores(tags, rec_span0, span3, n_rec, NC, ptr, pairs)
    full = TagCall(tags, rec_span0, span3, NC, ptr, pairs).run()
    _check_scores(full, want)
    mins = rs.uniform(0.3, 0.95, size=(K, NC)).astype(np.float32)
    mins[0, 0] = want[0] if not np.isnan(want[0]) else mins[0, 0]                # an exact tie: dropped
    w = sp.gate(ptr, pairs, want, n_rec, NC, mins)
    assert 0 < w[0][-1] < ptr[-1]
    k_point = SelectCall(ptr, pairs, full[0], None, n_rec, NC, mins).run()
    _check_gate(k_point, w)
    # the K-point call equals K one-point calls on the slices of ev_ptr
    span = n_rec * NC
    for k in range(K):
        sl = ptr[k * span:(k + 1) * span + 1]
        one = TagCall(tags, rec_span0, span3, NC, sl, pairs).run()
        a, b = int(sl[0]), int(sl[-1])
        assert one[1] == 0 and one[0][a:b].tobytes() == full[0][a:b].tobytes() and (np.delete(one[0], np.s_[a:b]) == SENTF).all()
        sel = SelectCall(sl, pairs, full[0], None, n_rec, NC, mins[k:k + 1]).run()
        n = int(sel[0][-1])
        np.testing.assert_array_equal(sel[0] - sel[0][0], k_point[0][k * span:(k + 1) * span + 1] - k_point[0][k * span])
        assert sel[1][:n].tobytes() == k_point[1][k_point[0][k * span]:k_point[0][(k + 1) * span]].tobytes()
    # min_tag = -inf returns the table byte for byte where no score is NaN
    clean = np.where(np.isnan(tags), np.float32(0.25), tags)
    score = TagCall(clean, rec_span0, span3, NC, ptr, pairs).run()[0]
    got = SelectCall(ptr, pairs, score, None, n_rec, NC, np.full((K, NC), -np.inf, np.float32)).run()
    n = int(ptr[-1])
    assert got[4] == 0 and got[0].tobytes() == ptr.tobytes() and got[1][:n].tobytes() == pairs[:n].tobytes()
    assert got[2][:n].tobytes() == score[:n].tobytes()


def _touch_counts():
    S = _short()
    return sorted({1, 2, S - 1, S, S + 1, 64, 65, 5000})


@pytest.mark.parametrize("span3", [1, 3])
def test_events_touching_1_to_5000_spans_and_the_span_boundaries(span3):
    """Spans touched on both sides of the thread / wave boundary and of a wave's stride.  Per count an event that starts on a
    span boundary and ends on one (it must not read the next span: that tag is the column's largest), one that starts and
    ends inside spans, and one reaching into the short last span."""
    S = _short()
    assert {S - 1, S, S + 1} == {31, 32, 33}
    NC, counts = 2, _touch_counts()
    L3 = sum(n * span3 + 2 * span3 for n in counts) * 2 + 200 * span3 + (1 if span3 > 1 else 0)
    rec_span0 = sp.span_table([L3, 40], span3)
    n_spans = int(rec_span0[1])
    tags = (_tags(3, int(rec_span0[-1]), NC) * np.float32(0.5)).astype(np.float32)
    aligned, inside, t = [], [], 0
    for n in counts:
        aligned.append((t * span3, (t + n) * span3))
        tags[t + n, 0] = 0.99                                                    # the span right behind it
        t += n + 1
    for n in counts:
        on = t * span3 + (span3 - 1)                                             # the last frame of span t ...
        inside.append((on, on + (n - 2) * span3 + 2 if n > 1 else on + 1))       # ... to the first frame of span t + n - 1
        t += n + 1
    assert t < n_spans - 2
    last = [((n_spans - 3) * span3, L3), (L3 - 1, L3)]                           # into and inside the short last span
    cols = [aligned, inside + last, [(0, 40)], []]
    ptr, pairs = _table(cols)
    want = sp.tag_scores(tags, rec_span0, span3, 2, NC, ptr, pairs)
    touched = [(off - 1) // span3 - on // span3 + 1 for on, off in aligned + inside]
    assert touched == counts + counts and (want[:len(counts)] < 0.5).all()
    _check_scores(TagCall(tags, rec_span0, span3, NC, ptr, pairs).run(), want)


def test_every_count_of_long_events_in_one_wave():
    """Wave w of the pairs array holds w events that their wave reduces (S + 1 spans), on lanes spread over the wave."""
    S, span3, NC = _short(), 1, 1
    rs = np.random.RandomState(6)
    n = np.full(65 * 64, 2)
    for w in range(65):
        n[w * 64 + rs.permutation(64)[:w]] = S + 1
    events, t = [], 1
    for k in n:
        events.append((t, t + int(k)))
        t += int(k) + 1
    L3 = t + 3
    rec_span0 = sp.span_table([L3], span3)
    tags = _tags(8, L3, NC, nan_every=500)
    ptr, pairs = _table([events])
    _check_scores(TagCall(tags, rec_span0, span3, NC, ptr, pairs).run(), sp.tag_scores(tags, rec_span0, span3, 1, NC, ptr, pairs))


@functools.lru_cache(maxsize=None)
def _big_table():
    """More than 1 024 workgroups of events: two columns of short events over spans of two frames, a few long ones."""
    rs = np.random.RandomState(2)
    n = rs.randint(1, 4, size=1024 * BLOCK + 700)
    n[[5, 70000, 140001, len(n) - 1]] = [5000, 130, 67, 300]
    cols, t = [[], []], [2, 2]
    for i, k in enumerate(n):
        c = 0 if i < 140000 else 1
        cols[c].append((t[c], t[c] + int(k)))
        t[c] += int(k) + 1
    span3, NC, L3 = 2, 2, max(t) + 1
    rec_span0 = sp.span_table([L3], span3)
    tags = _tags(3, int(rec_span0[-1]), NC, nan_every=1000)
    ptr, pairs = _table(cols)
    return tags, rec_span0, span3, NC, ptr, pairs, sp.tag_scores(tags, rec_span0, span3, 1, NC, ptr, pairs)


def test_more_than_1024_workgroups_twice_and_one_graph_replay():
    tags, rec_span0, span3, NC, ptr, pairs, want = _big_table()
    assert ptr[-1] > 1024 * BLOCK
    call = TagCall(tags, rec_span0, span3, NC, ptr, pairs)
    eager = call.run()
    _check_scores(eager, want)
    assert call.run()[0].tobytes() == eager[0].tobytes()
    graph = torch.cuda.CUDAGraph()
    call.fill()
    with torch.cuda.graph(graph):
        assert call.launch() == 0
    call.fill()
    graph.replay()
    replay = call.get()
    assert replay[1] == 0 and replay[0].tobytes() == eager[0].tobytes()
    mins = np.array([[0.5, 0.7]], np.float32)
    w = sp.gate(ptr, pairs, want, 1, NC, mins)
    assert 0.1 * ptr[-1] < w[0][-1] < 0.9 * ptr[-1]
    sel = SelectCall(ptr, pairs, eager[0], None, 1, NC, mins)
    s_eager = sel.run()
    _check_gate(s_eager, w)
    graph = torch.cuda.CUDAGraph()
    sel.fill()
    with torch.cuda.graph(graph):
        assert sel.launch() == 0
    sel.fill()
    graph.replay()
    s_replay = sel.get()
    assert s_replay[4] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(s_replay[:3], s_eager[:3]))


def test_nan_tags_are_skipped_and_an_all_nan_event_is_never_kept():
    S, span3, NC = _short(), 4, 2
    L3 = 4 * (S + 80)
    rec_span0 = sp.span_table([L3], span3)
    tags = _tags(4, int(rec_span0[-1]), NC)
    long_ = (S + 9) * span3
    cols = [[(0, 3), (8, 17), (40, 40 + long_), (40 + long_ + 4, 40 + 2 * long_ + 4)], [(1, 2), (5, 6)]]
    tags[2, 0] = np.nan                                                          # one of the three spans of (8, 17)
    tags[0, 0] = np.nan                                                          # the only span of (0, 3)
    tags[[10, 10 + S, 10 + S + 8], 0] = np.nan                                   # inside a long event: its first, a far and its last span
    lo = (40 + long_ + 4) // span3
    tags[lo:(40 + 2 * long_ + 3) // span3 + 1, 0] = np.nan                       # a whole long event
    tags[0, 1] = np.nan
    ptr, pairs = _table(cols)
    want = sp.tag_scores(tags, rec_span0, span3, 1, NC, ptr, pairs)
    assert np.isnan(want).tolist() == [True, False, False, True, True, False]
    out = TagCall(tags, rec_span0, span3, NC, ptr, pairs).run()
    _check_scores(out, want)
    got = SelectCall(ptr, pairs, out[0], None, 1, NC, [[-np.inf] * NC]).run()
    _check_gate(got, sp.gate(ptr, pairs, want, 1, NC, [[-np.inf] * NC]))
    assert got[0].tolist() == [0, 2, 3]


@pytest.mark.parametrize("event", [(10, 51), (7, 7), (9, 3), (-1, 4), (-5, -2), (2 ** 31 - 1, -2 ** 31)])
def test_an_event_outside_its_spans_raises_bit_64_and_scores_nan(event):
    """Recording 1 has 47 frames in 10 spans of 5: off = 51 is beyond S * span3 = 50 (48 .. 50 are not: the table's own bound)."""
    span3, NC, L3s = 5, 2, [300, 47, 500]
    rec_span0 = sp.span_table(L3s, span3)
    tags = _tags(9, int(rec_span0[-1]), NC)
    cols = [[(0, 3), (5, 250)], [(1, 2)], [(0, 40), (41, 50)], [(2, 9), (10, 30)], [(4, 5), (100, 400)], [(0, 500)]]
    cols[3][1] = event
    ptr, pairs = _table(cols)
    want = sp.tag_scores(tags, rec_span0, span3, 3, NC, ptr, pairs)
    i = int(ptr[3]) + 1
    assert np.isnan(want[i]) and np.isnan(want).sum() == 1
    out = TagCall(tags, rec_span0, span3, NC, ptr, pairs).run()
    _check_scores(out, want, err=64)
    got = SelectCall(ptr, pairs, out[0], None, 3, NC, [[-np.inf] * NC]).run()
    assert got[0][-1] == ptr[-1] - 1                                             # never kept


@pytest.mark.parametrize("what,entry,value", [("ptr", 1, -5), ("ptr", 6, 10 ** 6), ("span0", 1, 10 ** 6), ("span0", 0, -1),
                                              ("span0", 2, 50)])
def test_broken_columns_and_span_tables_raise_bit_16_and_leave_the_rest_right(what, entry, value):
    span3, NC, L3s = 5, 2, [300, 47, 500]
    rec_span0 = sp.span_table(L3s, span3)
    total = int(rec_span0[-1])
    tags = _tags(9, total, NC)
    cols = [[(0, 3), (5, 250)], [(1, 2)], [(0, 40), (41, 47)], [(2, 9), (10, 30)], [(4, 5), (100, 400)], [(0, 500)]]
    ptr, pairs = _table(cols)
    want = sp.tag_scores(tags, rec_span0, span3, 3, NC, ptr, pairs)
    bad_ptr, bad_s0 = ptr.copy(), rec_span0.copy()
    (bad_ptr if what == "ptr" else bad_s0)[entry] = value
    score, err = TagCall(tags, bad_s0, span3, NC, bad_ptr, pairs).run()
    assert err & 16 and not err & ~(16 | 64)
    for c in range(len(cols)):
        ix = np.arange(int(ptr[c]), int(ptr[c + 1]))
        rec = (c // NC) % 3
        col_ok = 0 <= bad_ptr[c] <= bad_ptr[c + 1] <= len(pairs)
        rec_ok = 0 <= bad_s0[rec] <= bad_s0[rec + 1] <= total
        if not col_ok or not rec_ok:
            assert (score[ix] == SENTF).all(), c                                 # nothing of it is read or written
        elif what == "ptr" or (bad_s0[rec] == rec_span0[rec] and bad_s0[rec + 1] == rec_span0[rec + 1]):
            _same_bits(score[ix], want[ix])


def test_bad_host_arguments_of_the_tag_scores_return_before_any_launch():
    span3, NC, L3s = 5, 2, [300, 47]
    rec_span0 = sp.span_table(L3s, span3)
    tags = _tags(9, int(rec_span0[-1]), NC)
    ptr, pairs = _table([[(0, 3)], [(1, 2)], [(0, 40)], []])
    call = TagCall(tags, rec_span0, span3, NC, ptr, pairs)
    call.fill()
    l = call.l
    assert call.launch(tags=None) != 0 and b"null" in l.sed_last_error()
    assert call.launch(score=None) != 0 and call.launch(s0=None) != 0 and call.launch(span3=0) != 0
    assert call.launch(NC=17) != 0 and call.launch(n_cols=5) != 0 and call.launch(cap=1 << 31) != 0 and call.launch(n_rec=0) != 0
    assert call.launch(total_spans=(1 << 31) // NC) != 0
    assert call.launch(score=call.tags) != 0 and b"overlaps" in l.sed_last_error()
    torch.cuda.synchronize()
    assert (call.score == SENT).all() and int(call.err[0].item()) == 0 and int(call.err[1].item()) == SENT


# ---- 4. end to end, small model ---------------------------------------------------------------------------------------------------
FRAME_S = 8 * 511 / 44100


@pytest.fixture(scope="module")
def e2e():
    from dcase2019_task4_amd.inference import LongRecordingSet, get_long_predictions, long_window_posteriors
    model, _ = gu.make_model(0)
    model.eval()
    names = ["a.wav", "b.wav", "c.wav", "d.wav"]
    ls = LongRecordingSet.from_arrays(_recordings([40, 64, 300, 900]), FRAMES, scaler=_Scaler(64), filenames=names)
    win_strong, win_att = long_window_posteriors(model, ls, 10, batch_size=8, want_attention=True)
    plain, timelines, _ = get_long_predictions(model, ls, LABELS, batch_size=8, return_posteriors=True)
    tl = torch.cat(timelines).cpu().numpy()
    thr = np.quantile(tl, 0.5, axis=0).astype(np.float32)
    return dict(model=model, ls=ls, win_strong=win_strong, win_att=win_att, tl=tl, thr=thr, names=names,
                kw=dict(batch_size=8, threshold=thr, median_window=3))


def _frame_of(out, ls, names):
    """The (label, onset frame, offset frame, filename) rows of a decoded one-point table."""
    ptr = out["ev_ptr"].cpu().numpy()
    ev = out["ev_pairs"].cpu().numpy()[:ptr[-1]]
    col = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return [(LABELS[c % 10], int(on), int(off), names[c // 10]) for c, (on, off) in zip(col, ev)]


def _rows(df):
    to_frame = lambda s: int(round(s / FRAME_S))
    return [(r.event_label, to_frame(r.onset), to_frame(r.offset), r.filename) for r in df.itertuples(index=False)]


def test_e2e_span_tags_equal_the_statement_and_the_frame_is_the_composition_by_hand(e2e):
    from dcase2019_task4_amd import inference as I
    model, ls, kw = e2e["model"], e2e["ls"], e2e["kw"]
    span_s, span3 = 3 * FRAME_S + 1e-6, 3
    df, (tags, rec_span0, got_span3) = I.get_long_predictions(model, ls, LABELS, tag_span=span_s, return_span_tags=True, **kw)
    assert got_span3 == span3 and tags.is_cuda and tuple(tags.shape) == (int(rec_span0[-1]), 10)
    np.testing.assert_array_equal(rec_span0, sp.span_table(np.diff(ls.rec_frame0_host), span3))
    want, _, _ = sp.pool(e2e["win_strong"].cpu().numpy(), e2e["win_att"].cpu().numpy(), ls.rec_win0_host, ls.rec_frame0_host,
                         ls.hop3, 1, span3)
    d = _ulps(tags.cpu().numpy(), want)
    print(f"{int((d != 0).sum())} of {want.size} span tags not bit-equal to the statement")
    assert (d <= 1).all()
    assert df.equals(I.get_long_predictions(model, ls, LABELS, **kw))             # tags alone gate nothing
    table = I.span_tags_dataframe(tags, rec_span0, span3, e2e["names"], LABELS, 0.5, FRAME_S, L3s=np.diff(ls.rec_frame0_host))
    assert len(table) == rec_span0[-1] and np.isclose(table.offset.iloc[-1], ls.durations()[-1], rtol=1e-12)
    # the order of the steps: decode + two-threshold select, gate, events_process, scores
    high = np.quantile(e2e["tl"], 0.8, axis=0).astype(np.float32)
    min_tag = np.quantile(want, 0.5, axis=0).astype(np.float32)
    extra = dict(threshold_high=high, min_event_length=0.3, min_event_gap=0.2, event_scores=True)
    got = I.get_long_predictions(model, ls, LABELS, tag_span=span_s, min_span_tag=min_tag, **extra, **kw)
    out = I.stitch_hysteresis(e2e["win_strong"], ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, [e2e["thr"]], [high],
                              [[3] * 10], "taper", ls.capacity(10), want_timeline=True)
    n_before = int(out["ev_ptr"][-1].item())
    span_tags = I.stitch_span_tags(e2e["win_strong"], e2e["win_att"], ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, span3)
    assert span_tags["tags"].cpu().numpy().tobytes() == tags.cpu().numpy().tobytes()
    out = I.gate_decoded(out, span_tags, ls.n_rec, 10, min_tag)
    assert 0 < int(out["ev_ptr"][-1].item()) < n_before
    min_len, max_gap = I.process_points([0.3], [0.2], 10, FRAME_S, 1)
    out = I.process_decoded(out, ls.n_rec, 10, min_len, max_gap)
    smax, smean, _ = I.events_scores(out, out["timeline"], ls.rec_frame0, ls.n_rec, 10)
    assert int(out["err"].item()) == 0
    rows = _frame_of(out, ls, e2e["names"])
    assert _rows(got) == rows and len(rows) > 0
    assert got.score_max.to_numpy().tobytes() == smax[:len(rows)].cpu().numpy().tobytes()
    assert got.score_mean.to_numpy().tobytes() == smean[:len(rows)].cpu().numpy().tobytes()


def test_e2e_a_very_large_span_is_the_recording_level_weak_mask(e2e):
    from dcase2019_task4_amd import inference as I
    model, ls, kw = e2e["model"], e2e["ls"], e2e["kw"]
    plain, weak = I.get_long_predictions(model, ls, LABELS, return_weak=True, **kw)
    weak = weak.cpu().numpy()
    min_tag = np.median(weak, axis=0).astype(np.float32)
    for span in (1e6, float("inf")):
        got, (tags, rec_span0, span3) = I.get_long_predictions(model, ls, LABELS, tag_span=span, min_span_tag=min_tag,
                                                               return_span_tags=True, **kw)
        assert span3 == int(np.diff(ls.rec_frame0_host).max()) and rec_span0.tolist() == [0, 1, 2, 3, 4]
        assert tags.cpu().numpy().tobytes() == weak.tobytes()
        keep = np.array([weak[e2e["names"].index(r.filename), LABELS.index(r.event_label)] > min_tag[LABELS.index(r.event_label)]
                         for r in plain.itertuples(index=False)])
        assert 0 < keep.sum() < len(plain)
        assert got.reset_index(drop=True)[["event_label", "onset", "offset", "filename"]].equals(
            plain[keep].reset_index(drop=True)[["event_label", "onset", "offset", "filename"]])


def test_e2e_defaults_are_unchanged_and_reach_no_new_entry(e2e, monkeypatch):
    from dcase2019_task4_amd import inference
    model, ls, kw = e2e["model"], e2e["ls"], e2e["kw"]
    before = inference.get_long_predictions(model, ls, LABELS, **kw)
    spelled = inference.get_long_predictions(model, ls, LABELS, tag_span=None, min_span_tag=None, return_span_tags=False, **kw)
    assert list(before.columns) == ["event_label", "onset", "offset", "filename"] and before.equals(spelled) and len(before) > 30

    def never(*a, **k):
        raise AssertionError("a new entry point was reached with the defaults")
    for name in ("stitch_span_tags", "events_tag_scores", "gate_decoded", "span_table"):
        monkeypatch.setattr(inference, name, never)
    l = inference._lib.lib()
    for name in ("sed_stitch_span_tags", "sed_events_tag_scores"):
        monkeypatch.setattr(l, name, never, raising=False)
    pd.testing.assert_frame_equal(inference.get_long_predictions(model, ls, LABELS, **kw), before)
    scored = inference.get_long_predictions(model, ls, LABELS, event_scores=True, min_event_length=0.2, **kw)
    assert len(scored) > 0


def _class_wise(pairs):
    return [(e.class_wise, s.class_wise, s.Ntn) for e, s in pairs]


def test_e2e_validate_long_with_the_gate(e2e, monkeypatch):
    from dcase2019_task4_amd import inference as I
    from dcase2019_task4_amd import metrics as M
    from tests.long_util import _ref_events
    model, ls = e2e["model"], e2e["ls"]
    rs = np.random.RandomState(5)
    cols = [[[(0.1, 0.4), (1.0, 2.5)] if rs.uniform() < 0.6 else [] for _ in range(10)] for _ in range(4)]
    ref = _ref_events(cols)
    ref.labels = LABELS
    thresholds = [0.5, e2e["thr"], float(np.median(e2e["tl"]))]
    K, span_s, span3 = 3, 3 * FRAME_S + 1e-6, 3
    base = dict(batch_size=8, min_event_lengths=[0.2], thresholds_high=None)
    plain = M.validate_long(model, ls, ref, thresholds, [3], **base)
    open_gate = M.validate_long(model, ls, ref, thresholds, [3], tag_span=span_s, min_span_tags=[-np.inf] * K, **base)
    assert _class_wise(open_gate) == _class_wise(plain)
    span_tags = I.stitch_span_tags(e2e["win_strong"], e2e["win_att"], ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, span3)
    tags = span_tags["tags"].cpu().numpy()
    mins = [float(np.quantile(tags, 0.5)), np.quantile(tags, 0.4, axis=0).astype(np.float32), 0.999]
    gated = M.validate_long(model, ls, ref, thresholds, [3], tag_span=span_s, min_span_tags=mins, **base)
    per_point = M.validate_long(model, ls, ref, thresholds, [3], tag_span=span_s, min_span_tags=mins, one_blend=False, **base)
    assert _class_wise(gated) == _class_wise(per_point) and _class_wise(gated) != _class_wise(plain)
    # the span tags are pooled ONCE per call; one gate per chunk, or one per point with one_blend=False
    calls = {"tags": 0, "gate": 0}
    pool_tags, gate = I.stitch_span_tags, I.gate_decoded
    monkeypatch.setattr(I, "stitch_span_tags", lambda *a, **k: (calls.__setitem__("tags", calls["tags"] + 1), pool_tags(*a, **k))[1])
    monkeypatch.setattr(I, "gate_decoded", lambda *a, **k: (calls.__setitem__("gate", calls["gate"] + 1), gate(*a, **k))[1])
    M.validate_long(model, ls, ref, thresholds, [3], tag_span=span_s, min_span_tags=mins, **base)
    assert calls == {"tags": 1, "gate": 1}
    M.validate_long(model, ls, ref, thresholds, [3], tag_span=span_s, min_span_tags=mins, one_blend=False, **base)
    assert calls == {"tags": 2, "gate": 1 + K}
    M.validate_long(model, ls, ref, thresholds, [3], **base)
    assert calls == {"tags": 2, "gate": 1 + K}
    monkeypatch.undo()
    one = M.validate_long(model, ls, ref, thresholds, [3], tag_span=span_s, min_span_tags=mins[:1], **base)
    assert _class_wise(one)[0] == _class_wise(gated)[0]
    # by hand: one sweep, the gate, events_process, long_sweep_event_counts
    thr, win = I.sweep_points(thresholds, [3], 10)
    out = I.stitch_sweep(e2e["win_strong"], ls.rec_win0, ls.rec_frame0, ls.total_frames, ls.hop3, torch.from_numpy(thr).cuda(),
                         torch.from_numpy(win).cuda(), "taper", K * ls.capacity(10))
    n_before = int(out["ev_ptr"][-1].item())
    min_tag = np.stack([np.broadcast_to(np.asarray(m, np.float32), (10,)) for m in mins])
    out = I.gate_decoded(out, span_tags, ls.n_rec, 10, min_tag)
    assert 0 < int(out["ev_ptr"][-1].item()) < n_before
    min_len, max_gap = I.process_points([0.2], None, 10, FRAME_S, K)
    out = I.process_decoded(out, ls.n_rec, 10, min_len, max_gap)
    counts = M.Counts(K, 10, "cuda")
    M.long_sweep_event_counts(out, ref, ls.pooling_time_ratio, counts=counts)
    ev, seg = counts.host()
    assert _class_wise(M._metric_pairs(LABELS, ev, seg)) == _class_wise(gated)
    # with a two-threshold decode in front of it
    high = [max(0.7, float(np.max(e2e["thr"])) + 0.1)]
    hyst = M.validate_long(model, ls, ref, thresholds, [3], batch_size=8, thresholds_high=high, tag_span=span_s, min_span_tags=[-np.inf])
    assert _class_wise(hyst) == _class_wise(M.validate_long(model, ls, ref, thresholds, [3], batch_size=8, thresholds_high=high))

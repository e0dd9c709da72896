"""-m gpu tests of the two-threshold (hysteresis) decode: sed_events_hysteresis alone on hand-made event tables (edges of the
rule, workgroup edges, a scan of more than 1024 workgroup counts, the error bits, two calls, one graph replay), the sweep +
select pipeline exact against tests/hysteresis_np.py, and the Python entry points (inference.stitch_hysteresis,
get_long_predictions(threshold_high=...), metrics.validate_long(thresholds_high=...)).  Every buffer a kernel writes starts as
sentinel bytes and carries a tail that must come back untouched; the workspace starts as 0xFF bytes."""
import functools

import numpy as np
import pytest
import torch

from tests import gpu_util as gu
from tests import hysteresis_np as hy
from tests import long_score_np as ls
from tests import sed_eval_np as se
from tests import stitch_np
from tests.hysteresis_np import smooth_timeline
from tests.long_util import SENT, TAIL, StitchCall, _group, _Scaler, _tables, _tile

pytestmark = pytest.mark.gpu

NUM, DEN = 8.0, 44100 / 511
BLOCK = 256                                                                    # indices per workgroup of the flat passes


class HystCall:
    """One sed_events_hysteresis call on sentinel-filled outputs (-7 integers) and a 0xFF workspace, each with a tail of TAIL
    elements that ``get()`` checks.  ``lo_ptr`` / ``hi_ptr`` / ``pairs``: numpy arrays or device tensors."""

    def __init__(self, lo_ptr, hi_ptr, pairs, out_capacity=None):
        from dcase2019_task4_amd import _lib
        self._lib, self.l = _lib, _lib.lib()
        dev = lambda a, dt: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
        self.lo_ptr, self.hi_ptr = dev(lo_ptr, np.int64), dev(hi_ptr, np.int64)
        self.pairs = dev(np.asarray(pairs).reshape(-1, 2) if not torch.is_tensor(pairs) else pairs, np.int32)
        self.n_cols, self.cap = self.lo_ptr.numel() - 1, self.pairs.shape[0]
        if self.cap == 0:
            self.pairs = torch.full((1, 2), SENT, dtype=torch.int32, device="cuda")              # (an address; no row is given)
        self.out_cap = self.cap if out_capacity is None else int(out_capacity)
        self.out_ptr = torch.empty(self.n_cols + 1 + TAIL, dtype=torch.int64, device="cuda")
        self.out_pairs = torch.empty(self.out_cap + TAIL, 2, dtype=torch.int32, device="cuda")
        self.err = torch.empty(2, dtype=torch.int32, device="cuda")
        self.ws_bytes = self.l.sed_events_hysteresis_ws_bytes(self.cap, self.n_cols)
        assert self.ws_bytes > 0, self.l.sed_last_error()
        self.ws = torch.empty(self.ws_bytes + TAIL, dtype=torch.uint8, device="cuda")

    def fill(self, err0=0):
        self.out_ptr.fill_(SENT)
        self.out_pairs.fill_(SENT)
        self.ws.fill_(0xFF)
        self.err.fill_(SENT)
        self.err[:1].fill_(err0)

    def launch(self, **kw):
        p = self._lib.ptr
        a = dict(cap=self.cap, n_cols=self.n_cols, ws_bytes=self.ws_bytes, lo_ptr=self.lo_ptr, out_pairs=self.out_pairs)
        a.update(kw)
        return self.l.sed_events_hysteresis(p(a["lo_ptr"]), p(self.hi_ptr), p(self.pairs), a["cap"], a["n_cols"], p(self.out_ptr),
                                            p(a["out_pairs"]), self.out_cap, p(self.ws), a["ws_bytes"], p(self.err),
                                            self._lib.stream_ptr())

    def get(self):
        torch.cuda.synchronize()
        out_ptr, out_pairs = self.out_ptr.cpu().numpy(), self.out_pairs.cpu().numpy()
        assert (out_ptr[self.n_cols + 1:] == SENT).all() and (out_pairs[self.out_cap:] == SENT).all()
        assert int(self.err[1].item()) == SENT and (self.ws[-TAIL:] == 0xFF).all()
        return out_ptr[:self.n_cols + 1], out_pairs[:self.out_cap], int(self.err[0].item())

    def run(self, err0=0):
        self.fill(err0)
        assert self.launch() == 0, self.l.sed_last_error()
        return self.get()


def _table(lo_cols, hi_cols, pad=3):
    """Two lists of columns (lists of (on, off)) as one pairs array [lo events | hi events | pad sentinel rows] and its two
    CSR offset arrays - the layout a sweep of [lo, hi] points leaves."""
    assert len(lo_cols) == len(hi_cols)
    n_lo = sum(len(c) for c in lo_cols)
    lo_ptr = np.r_[0, np.cumsum([len(c) for c in lo_cols])].astype(np.int64)
    hi_ptr = (n_lo + np.r_[0, np.cumsum([len(c) for c in hi_cols])]).astype(np.int64)
    rows = [e for c in lo_cols for e in c] + [e for c in hi_cols for e in c] + [(SENT, SENT)] * pad
    return lo_ptr, hi_ptr, np.asarray(rows, dtype=np.int32).reshape(-1, 2)


def _select_fast(lo_ptr, hi_ptr, pairs):
    """The rule per column with searchsorted (for tables too large for the double loop; pinned to it on the small ones)."""
    ptr, kept = [0], []
    for c in range(len(lo_ptr) - 1):
        lo, hi_on = pairs[lo_ptr[c]:lo_ptr[c + 1]], pairs[hi_ptr[c]:hi_ptr[c + 1], 0]
        j = np.searchsorted(hi_on, lo[:, 0], side="left")
        ok = (j < len(hi_on)) & (hi_on[np.minimum(j, max(len(hi_on) - 1, 0))] < lo[:, 1]) if len(hi_on) else np.zeros(len(lo), bool)
        kept.append(lo[ok])
        ptr.append(ptr[-1] + int(ok.sum()))
    return np.asarray(ptr, np.int64), np.concatenate(kept).astype(np.int32).reshape(-1, 2)


def _check(call_out, want):
    out_ptr, out_pairs, err = call_out
    assert err == 0
    np.testing.assert_array_equal(out_ptr, want[0])
    np.testing.assert_array_equal(out_pairs[:out_ptr[-1]], want[1])
    assert (out_pairs[out_ptr[-1]:] == SENT).all()                             # nothing beyond the true count


def _columns(out_ptr, out_pairs):
    return [[tuple(int(v) for v in e) for e in out_pairs[out_ptr[c]:out_ptr[c + 1]]] for c in range(len(out_ptr) - 1)]


# ---- 1. the entry alone, on hand-made tables --------------------------------------------------------------------------------------
def _edge_table():
    lo = [[],                                                                  # empty low, empty high
          [(0, 4), (10, 12)],                                                  # no high event at all: none kept
          [],                                                                  # (a high event without a low one cannot come from a decode)
          [(2, 6), (8, 9), (20, 30), (31, 33)],                                # all kept
          [(5, 10), (10, 15), (20, 25)],                                       # on_hi == on is kept; on_hi == off is not
          [(0, 100)],                                                          # several high events in one low event
          [(0, 3), (5, 8), (10, 13), (15, 18)]]                                # alternately kept
    hi = [[], [], [], [(3, 5), (8, 9), (25, 26), (32, 33)], [(5, 6), (15, 16)], [(1, 2), (50, 60), (99, 100)], [(6, 7), (16, 17)]]
    return lo, hi


def test_the_rule_at_its_edges_twice_with_identical_bytes():
    lo, hi = _edge_table()
    lo_ptr, hi_ptr, pairs = _table(lo, hi)
    want = hy.select(lo_ptr, pairs, hi_ptr, pairs)
    assert _columns(*want) == [[], [], [], lo[3], [(5, 10)], [(0, 100)], [(5, 8), (15, 18)]]
    fast = _select_fast(lo_ptr, hi_ptr, pairs)
    assert fast[0].tobytes() == want[0].tobytes() and fast[1].tobytes() == want[1].tobytes()
    call = HystCall(lo_ptr, hi_ptr, pairs)
    first = call.run()
    _check(first, want)
    second = call.run()
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    # the same table as its own high table keeps everything: lo_ptr given twice
    same = HystCall(lo_ptr, lo_ptr, pairs).run()
    _check(same, (lo_ptr - lo_ptr[0], pairs[:lo_ptr[-1]]))
    # a given error word is OR-ed into
    assert call.run(err0=32)[2] == 32


def test_empty_tables_and_zero_capacity():
    z = np.zeros(4, np.int64)
    out_ptr, out_pairs, err = HystCall(z, z, np.zeros((0, 2), np.int32)).run()          # no rows at all: the flag pass has no grid
    assert err == 0 and (out_ptr == 0).all() and out_pairs.shape[0] == 0
    out_ptr, _, err = HystCall(z, z, np.full((5, 2), SENT, np.int32)).run()             # capacity without events
    assert err == 0 and (out_ptr == 0).all()


@pytest.mark.parametrize("n_kept", [255, 256, 257])
def test_kept_counts_around_a_workgroup_with_column_edges_on_workgroup_edges(n_kept):
    ev = lambda k: (10 * k, 10 * k + 7)
    col0 = [ev(k) for k in range(BLOCK)]                                       # fills workgroup 0 exactly; every second one kept
    col1 = [ev(k) for k in range(2 * BLOCK)]                                   # workgroups 1 and 2: the first n_kept kept
    col2 = [ev(k) for k in range(3)]                                           # starts on a workgroup edge
    hi = [[(10 * k + 3, 10 * k + 5) for k in range(0, BLOCK, 2)], [(10 * k, 10 * k + 1) for k in range(n_kept)], [(26, 27)]]
    lo_ptr, hi_ptr, pairs = _table([col0, col1, col2], hi, pad=0)
    assert lo_ptr.tolist() == [0, BLOCK, 3 * BLOCK, 3 * BLOCK + 3]
    want = hy.select(lo_ptr, pairs, hi_ptr, pairs)
    assert np.diff(want[0]).tolist() == [BLOCK // 2, n_kept, 1]
    _check(HystCall(lo_ptr, hi_ptr, pairs).run(), want)
    # ... and the kept events themselves end on a workgroup edge of the input: one column of exactly n_kept events, all kept
    lo_ptr, hi_ptr, pairs = _table([col1[:n_kept]], [[(a, a + 1) for a, _ in col1[:n_kept]]], pad=0)
    _check(HystCall(lo_ptr, hi_ptr, pairs).run(), (lo_ptr, pairs[:n_kept]))


@functools.lru_cache(maxsize=None)
def _big_table():
    """600 columns of 450 low events (270 000: 1055 workgroups of the flat pass, the count scan loops twice), about half of them
    confirmed, a few columns empty."""
    rs = np.random.RandomState(5)
    lo, hi = [], []
    for c in range(600):
        n = 0 if c % 97 == 5 else 450
        on = np.cumsum(rs.randint(3, 9, size=n))
        length = rs.randint(1, 3, size=n)
        keep = rs.uniform(size=n) < 0.5
        lo.append(np.stack([on, on + length], 1))
        shift = rs.randint(0, 2, size=n) * (length - 1)                        # the high onset anywhere inside the low event
        hi.append(np.stack([on + shift, on + shift + 1], 1)[keep])
    lo_ptr = np.r_[0, np.cumsum([len(c) for c in lo])].astype(np.int64)
    hi_ptr = (lo_ptr[-1] + np.r_[0, np.cumsum([len(c) for c in hi])]).astype(np.int64)
    pairs = np.concatenate(lo + hi + [np.full((100, 2), SENT)]).astype(np.int32)
    return lo_ptr, hi_ptr, pairs, _select_fast(lo_ptr, hi_ptr, pairs)


def test_more_than_1024_workgroups_of_events_and_one_graph_replay():
    lo_ptr, hi_ptr, pairs, want = _big_table()
    assert lo_ptr[-1] > 1024 * BLOCK and 0.4 < want[0][-1] / lo_ptr[-1] < 0.6
    call = HystCall(lo_ptr, hi_ptr, pairs)
    eager = call.run()
    _check(eager, want)
    graph = torch.cuda.CUDAGraph()
    call.fill()
    with torch.cuda.graph(graph):
        assert call.launch() == 0
    call.fill()
    graph.replay()
    replay = call.get()
    assert replay[2] == 0 and replay[0].tobytes() == eager[0].tobytes() and replay[1].tobytes() == eager[1].tobytes()


def test_one_kept_event_too_many_raises_bit_2_and_writes_nothing_beyond():
    lo_ptr, hi_ptr, pairs, want = _big_table()
    n = int(want[0][-1])
    out_ptr, out_pairs, err = HystCall(lo_ptr, hi_ptr, pairs, out_capacity=n - 1).run()          # (get() checks the tail behind it)
    assert err == 2
    np.testing.assert_array_equal(out_ptr, want[0])                            # ALWAYS the true counts
    _check(HystCall(lo_ptr, hi_ptr, pairs, out_capacity=n).run(), want)


@pytest.mark.parametrize("which,value", [("hi", -5), ("hi", 10 ** 6), ("hi", "decreasing"), ("lo_last", 10 ** 6), ("lo_first", -2)])
def test_broken_offsets_raise_bit_16_and_leave_the_other_columns_right(which, value):
    lo, hi = _edge_table()
    lo_ptr, hi_ptr, pairs = _table(lo, hi)
    want = _columns(*hy.select(lo_ptr, pairs, hi_ptr, pairs))
    lo_ptr, hi_ptr = lo_ptr.copy(), hi_ptr.copy()
    undefined = ()
    if which == "hi" and value == "decreasing":                                # column 3 ends in front of its start: skipped; column
        hi_ptr[4], skipped, undefined = hi_ptr[3] - 1, (3,), (4,)              # 4 has valid bounds that are not its own
    elif which == "hi":                                                        # entry 4 bounds the columns 3 and 4
        hi_ptr[4], skipped = value, (3, 4)
    elif which == "lo_last":
        lo_ptr[-1], skipped = value, (len(lo) - 1,)
    else:
        lo_ptr[0], skipped = value, (0,)
    out_ptr, out_pairs, err = HystCall(lo_ptr, hi_ptr, pairs).run()
    assert err & 16 and not err & ~(16 | 64)
    got = _columns(out_ptr, out_pairs)
    for c in range(len(lo)):
        if c in undefined:
            continue
        assert got[c] == ([] if c in skipped else want[c]), c


@pytest.mark.parametrize("side", ["lo", "hi"])
def test_onsets_out_of_order_raise_bit_64_and_leave_the_other_columns_right(side):
    lo, hi = _edge_table()
    lo_ptr, hi_ptr, pairs = _table(lo, hi)
    want = _columns(*hy.select(lo_ptr, pairs, hi_ptr, pairs))
    i = int(lo_ptr[3] if side == "lo" else hi_ptr[3])                          # column 3: its first two events swapped
    orig, pairs = pairs, pairs.copy()
    pairs[[i, i + 1]] = pairs[[i + 1, i]]
    out_ptr, out_pairs, err = HystCall(lo_ptr, hi_ptr, pairs).run()
    assert err == 64
    got = _columns(out_ptr, out_pairs)
    assert [g for c, g in enumerate(got) if c != 3] == [w for c, w in enumerate(want) if c != 3]
    equal = orig.copy()                                                        # equal onsets are not strictly increasing either
    equal[i + 1, 0] = equal[i, 0]
    assert HystCall(lo_ptr, hi_ptr, equal).run()[2] == 64


def test_bad_host_arguments_return_before_any_launch():
    lo, hi = _edge_table()
    call = HystCall(*_table(lo, hi))
    call.fill()
    l = call.l
    assert l.sed_events_hysteresis_ws_bytes(1 << 31, 4) == 0 and l.sed_events_hysteresis_ws_bytes(8, 1 << 26) == 0
    assert l.sed_events_hysteresis_ws_bytes(-1, 4) == 0 and l.sed_events_hysteresis_ws_bytes(8, 0) == 0
    assert call.launch(lo_ptr=None) != 0 and b"null" in l.sed_last_error()
    assert call.launch(cap=1 << 31) != 0 and call.launch(n_cols=0) != 0
    assert call.launch(ws_bytes=call.ws_bytes + 8) != 0 and b"ws_bytes" in l.sed_last_error()
    assert call.launch(out_pairs=call.pairs) != 0
    torch.cuda.synchronize()
    assert (call.out_ptr == SENT).all() and (call.out_pairs == SENT).all() and int(call.err[0].item()) == 0


# ---- 2. end to end against the numpy statement, exact ---------------------------------------------------------------------------------
# The grid's windows stop at 15 because its tables hold a recording of 2 frames: where a window has 8 L + 1 frames or more and
# L is even, scipy's median filter (the statement's) leaves the periodic reflection that include/dcase_sed.h defines and the
# kernels follow - at L = 2 from window 17 on.  The widest window runs on the "wide" tables, which hold 3 frames instead.
T3_E = 16
WINDOWS = {False: [1, 3, 8, 15], True: [1, 3, 8, 63]}


def _e2e_lengths(wide):
    t = _tile()
    return [1, 3 if wide else 2, t - 1, t, t + 1, 1100]


@functools.lru_cache(maxsize=None)
def _e2e_blend(NC, hop3, wide=False):
    """Window posteriors that are slices of one smooth random timeline per recording plus a little noise (so the blend
    matters), their tables and the numpy blend."""
    L3s = _e2e_lengths(wide)
    rec_win0, rec_frame0 = _tables(L3s, T3_E, hop3)
    rs = np.random.RandomState(7 + 10 * NC + hop3)
    p = rs.uniform(size=(rec_win0[-1], T3_E, NC)).astype(np.float32)             # (the tails beyond a recording's end stay noise)
    for r, L in enumerate(L3s):
        base = smooth_timeline(300 + 10 * r + NC, L, NC)
        for j in range(rec_win0[r + 1] - rec_win0[r]):
            n = min(T3_E, L - j * hop3)
            noise = rs.uniform(-0.02, 0.02, size=(n, NC)).astype(np.float32)
            p[rec_win0[r] + j, :n] = base[j * hop3:j * hop3 + n] + noise
    return p, rec_win0, rec_frame0, stitch_np.blend(p, rec_win0, rec_frame0, hop3, 1)


@functools.lru_cache(maxsize=None)
def _e2e_case(NC, hop3, K, wide=False):
    """Thresholds from the timeline's quantiles, chosen on the CPU; the statement's table and its low decode."""
    p, rec_win0, rec_frame0, tl = _e2e_blend(NC, hop3, wide)
    rs = np.random.RandomState(K)
    q_lo, q_hi = rs.uniform(0.3, 0.6, size=(K, 1)), rs.uniform(0.7, 0.97, size=(K, 1))
    thr_lo = np.stack([np.quantile(tl, q, axis=0) for q in q_lo[:, 0]]).astype(np.float32)
    thr_hi = np.maximum(np.stack([np.quantile(tl, q, axis=0) for q in q_hi[:, 0]]).astype(np.float32), thr_lo)
    win = rs.choice(WINDOWS[wide], size=(K, NC)).astype(np.int32)
    if K > 1:
        thr_hi[1] = thr_lo[1]                                                  # one pair that keeps everything
    ev_ptr, ev_pairs = hy.decode_pairs(tl, rec_frame0, thr_lo, thr_hi, win)
    n_low = sum(int(stitch_np.decode(tl, rec_frame0, thr_lo[k], win[k])[1][-1]) for k in range(K) if K == 1 or k != 1)
    n_kept = int(ev_ptr[-1]) - (int(ev_ptr[2 * (len(rec_frame0) - 1) * NC] - ev_ptr[(len(rec_frame0) - 1) * NC]) if K > 1 else 0)
    return thr_lo, thr_hi, win, ev_ptr, ev_pairs, n_low, n_kept


GRID = [(NC, hop3, K, False) for NC in (3, 4) for hop3 in (8, 16) for K in (1, 3, 9)]
WIDE = [(3, 8, 3, True), (4, 16, 9, True)]


def test_the_grid_exercises_both_branches_of_the_rule():
    """Over the grid (without the pairs whose thresholds are equal) the statement alone keeps at least 10 % and drops at least
    10 % of the low events."""
    low = sum(_e2e_case(*g)[5] for g in GRID)
    kept = sum(_e2e_case(*g)[6] for g in GRID)
    assert low > 500 and kept >= 0.1 * low and low - kept >= 0.1 * low, (low, kept)


@pytest.mark.parametrize("NC,hop3,K,wide", GRID + WIDE)
def test_sweep_and_select_are_the_numpy_statement(NC, hop3, K, wide):
    p, rec_win0, rec_frame0, tl = _e2e_blend(NC, hop3, wide)
    thr_lo, thr_hi, win, want_ptr, want_pairs, _, _ = _e2e_case(NC, hop3, K, wide)
    assert wide == bool((win == 63).any())
    assert K != 9 or 2 * K > 2 * _group()                                      # 18 points: more than two point groups
    sweep = StitchCall(p, rec_win0, rec_frame0, hop3, 1, np.concatenate([thr_lo, thr_hi]), np.concatenate([win, win]), sweep=True)
    out = sweep.run()
    assert out["err"] == 0
    n_cols = K * (len(rec_frame0) - 1) * NC
    call = HystCall(sweep.ev_ptr[:n_cols + 1], sweep.ev_ptr[n_cols:2 * n_cols + 1], sweep.ev_pairs[:sweep.capacity],
                    out_capacity=sweep.capacity // 2)
    _check(call.run(), (want_ptr, want_pairs))
    # the Python entry: the same table, the error word of both calls in one
    from dcase2019_task4_amd.inference import stitch_hysteresis
    res = stitch_hysteresis(torch.from_numpy(p).cuda(), torch.from_numpy(rec_win0).cuda(), torch.from_numpy(rec_frame0).cuda(),
                            int(rec_frame0[-1]), hop3, list(thr_lo), list(thr_hi), list(win))
    assert int(res["err"].item()) == 0 and res["n_points"] == K and res["ev_ptr"].numel() == n_cols + 1
    ptr = res["ev_ptr"].cpu().numpy()
    np.testing.assert_array_equal(ptr, want_ptr)
    np.testing.assert_array_equal(res["ev_pairs"].cpu().numpy()[:ptr[-1]], want_pairs)


@pytest.mark.parametrize("NC,hop3", [(3, 8), (4, 16)])
def test_equal_thresholds_are_sed_stitch_decode_byte_for_byte(NC, hop3):
    p, rec_win0, rec_frame0, tl = _e2e_blend(NC, hop3)
    thr, _, win, _, _, _, _ = _e2e_case(NC, hop3, 1)
    dec = StitchCall(p, rec_win0, rec_frame0, hop3, 1, thr, win).run()
    assert dec["err"] == 0 and dec["ev_ptr"][-1] > 20
    sweep = StitchCall(p, rec_win0, rec_frame0, hop3, 1, np.concatenate([thr, thr]), np.concatenate([win, win]), sweep=True)
    assert sweep.run()["err"] == 0
    n_cols = (len(rec_frame0) - 1) * NC
    out_ptr, out_pairs, err = HystCall(sweep.ev_ptr[:n_cols + 1], sweep.ev_ptr[n_cols:2 * n_cols + 1],
                                       sweep.ev_pairs[:sweep.capacity], out_capacity=dec["ev_pairs"].shape[0] - TAIL).run()
    n = int(dec["ev_ptr"][-1])
    assert err == 0 and out_ptr.tobytes() == dec["ev_ptr"].tobytes() and out_pairs[:n].tobytes() == dec["ev_pairs"][:n].tobytes()


def test_a_sweep_error_reaches_the_result_word():
    from dcase2019_task4_amd.inference import stitch_hysteresis
    p, rec_win0, rec_frame0, tl = _e2e_blend(3, 8)
    thr_lo, thr_hi, win, _, _, _, _ = _e2e_case(3, 8, 1)
    dev = lambda a: torch.from_numpy(a).cuda()
    res = stitch_hysteresis(dev(p), dev(rec_win0), dev(rec_frame0), int(rec_frame0[-1]), 8, list(thr_lo), list(thr_hi), [64])
    assert int(res["err"].item()) & 8                                          # the sweep's bit: a window outside 1 .. 63
    res = stitch_hysteresis(dev(p), dev(rec_win0), dev(rec_frame0), int(rec_frame0[-1]), 8, list(thr_lo), list(thr_hi), list(win),
                            capacity=2)
    assert int(res["err"].item()) & 2                                          # the sweep's table overflowed: nothing is addressed beyond it


# ---- 3. through the Python entry points -----------------------------------------------------------------------------------------------
def _seconds_columns(ev_ptr, ev_pairs, n_rec, NC, k=0):
    return [[[(int(a) * NUM / DEN, int(b) * NUM / DEN) for a, b in ev_pairs[ev_ptr[(k * n_rec + r) * NC + c]:ev_ptr[(k * n_rec + r) * NC + c + 1]]]
             for c in range(NC)] for r in range(n_rec)]


def test_validate_long_and_get_long_predictions_with_a_high_threshold():
    from dcase2019_task4_amd import metrics as M
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
    f0 = lset.rec_frame0_host
    K, n_rec, NC = 3, 3, 10
    thr_lo = np.stack([np.quantile(tl, q, axis=0) for q in (0.4, 0.5, 0.6)]).astype(np.float32)
    thr_hi = np.stack([np.quantile(tl, q, axis=0) for q in (0.8, 0.7, 0.9)]).astype(np.float32)
    win = np.array([[3, 1, 5, 3, 3, 7, 3, 1, 3, 5], [1] * 10, [5] * 10], np.int32)
    want_ptr, want_pairs = hy.decode_pairs(tl, f0, thr_lo, thr_hi, win)
    low = sum(int(stitch_np.decode(tl, f0, thr_lo[k], win[k])[1][-1]) for k in range(K))
    assert 0 < want_ptr[-1] < low                                              # something is kept and something is dropped
    cols = [_seconds_columns(want_ptr, want_pairs, n_rec, NC, k) for k in range(K)]
    ref_cols = ls.sorted_jittered_references(cols[0], 6)
    pack = lambda c: M.RefEvents(*ls.pack(c), names, labels)
    ref, ests = pack(ref_cols), [pack(c) for c in cols]
    # the integers of the from_events scorers on the numpy-selected tables
    c_w = M.long_sweep_event_counts_from_events(ests, ref)
    e_w = M.long_sweep_error_from_events(ests, ref)
    p_w = M.long_sweep_psds_counts_from_events(ests, ref)
    want = M._metric_pairs(labels, *c_w.host(), e_w.host())
    thr, high, wins = list(thr_lo), list(thr_hi), list(win)
    cap = lset.capacity(NC)
    for kw in (dict(), dict(max_table_bytes=8 * cap * 2)):                     # one chunk of three pairs; one pair per chunk
        psds = M.PSDSCounts(K, NC, "cuda")
        got = M.validate_long(model, lset, ref, thr, wins, batch_size=8, psds=psds, error_rate=True, thresholds_high=high, **kw)
        for k in range(K):
            for i in (0, 1):
                assert got[k][i].class_wise == want[k][i].class_wise and got[k][i].overall_sdi == want[k][i].overall_sdi, (kw, k, i)
            assert got[k][1].Ntn == want[k][1].Ntn
        assert psds.host().tobytes() == p_w.host().tobytes()
    # a high threshold equal to the low one: the integers of the plain call (one entry is broadcast)
    same = M.validate_long(model, lset, ref, thr[:1], wins[:1], batch_size=8, thresholds_high=thr[:1])
    base = M.validate_long(model, lset, ref, thr[:1], wins[:1], batch_size=8)
    assert same[0][0].class_wise == base[0][0].class_wise and same[0][1].class_wise == base[0][1].class_wise
    one = M.validate_long(model, lset, ref, thr, wins, batch_size=8, thresholds_high=[[1.0] * NC])      # nothing is confirmed
    assert all(v["Nsys"] == 0 for k in range(K) for v in one[k][0].class_wise.values())
    with pytest.raises(ValueError, match="one_blend"):
        M.validate_long(model, lset, ref, thr, wins, one_blend=False, thresholds_high=high)
    with pytest.raises(ValueError, match="thr_hi >= thr_lo"):
        M.validate_long(model, lset, ref, thr, wins, thresholds_high=[0.0])
    # get_long_predictions: the DataFrame of the statement at pair 0
    df = get_long_predictions(model, lset, labels, batch_size=8, threshold=thr_lo[0], median_window=win[0], threshold_high=thr_hi[0])
    got_cols = se.columns_from_rows(df[["event_label", "onset", "offset", "filename"]].itertuples(index=False), names, labels)
    assert got_cols == cols[0] and 0 < len(df) < len(get_long_predictions(model, lset, labels, batch_size=8, threshold=thr_lo[0],
                                                                          median_window=win[0]))
    with pytest.raises(ValueError, match="thr_hi >= thr_lo"):
        get_long_predictions(model, lset, labels, threshold=0.5, threshold_high=0.4)


def test_clip_batches_are_one_window_recordings():
    """A batch of clip posteriors [n, T, NC] through stitch_hysteresis: n one-window recordings, no path of their own."""
    from dcase2019_task4_amd.inference import stitch_hysteresis
    n, T, NC = 5, 157, 4
    p = np.stack([smooth_timeline(70 + i, T, NC) for i in range(n)])
    rec_win0, rec_frame0 = np.arange(n + 1, dtype=np.int32), np.arange(n + 1, dtype=np.int64) * T
    thr_lo, thr_hi, win = np.full((1, NC), 0.4, np.float32), np.full((1, NC), 0.8, np.float32), np.array([[1, 3, 8, 63]], np.int32)
    want_ptr, want_pairs = hy.decode_pairs(p.reshape(n * T, NC), rec_frame0, thr_lo, thr_hi, win)
    lo_events = int(stitch_np.decode(p.reshape(n * T, NC), rec_frame0, thr_lo[0], win[0])[1][-1])
    assert 0 < want_ptr[-1] < lo_events
    res = stitch_hysteresis(torch.from_numpy(p).cuda(), torch.from_numpy(rec_win0).cuda(), torch.from_numpy(rec_frame0).cuda(),
                            n * T, T, list(thr_lo), list(thr_hi), list(win))
    assert int(res["err"].item()) == 0
    ptr = res["ev_ptr"].cpu().numpy()
    np.testing.assert_array_equal(ptr, want_ptr)
    np.testing.assert_array_equal(res["ev_pairs"].cpu().numpy()[:ptr[-1]], want_pairs)

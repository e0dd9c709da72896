"""-m gpu tests of minimum event length and gap merging: sed_events_process alone on hand-made event tables (wave, workgroup
and scan-strip edges, chains and runs of dropped events across them, column starts, the error bits, two calls, one graph
replay), on the tables of sed_stitch_sweep, and through the Python entry points (inference.events_process,
get_long_predictions(min_event_length=..., min_event_gap=...), metrics.validate_long(min_event_lengths=...,
min_event_gaps=...)).  Every case demands exact equality with tests/event_process_np.py: out_ptr and
out_pairs[:out_ptr[-1]].  Every buffer a kernel writes starts as sentinel bytes and carries a tail that must come back
untouched; the workspace starts as 0xFF bytes."""
import functools

import numpy as np
import pytest
import torch

from tests import event_process_np as ep
from tests import gpu_util as gu
from tests import hysteresis_np as hy
from tests import long_score_np as ls
from tests import sed_eval_np as se
from tests import stitch_np
from tests.hysteresis_np import smooth_timeline
from tests.long_util import SENT, TAIL, StitchCall, _Scaler, _tables

pytestmark = pytest.mark.gpu

NUM, DEN = 8.0, 44100 / 511
BLOCK = 256                                                                    # indices per workgroup of the flat passes
STRIP = 1024                                                                   # workgroup values per strip of the scans
ORDERS = [0, 1]


class ProcCall:
    """One sed_events_process call on sentinel-filled outputs (-7 integers) and a 0xFF workspace, each with a tail of TAIL
    elements that ``get()`` checks.  ``ev_ptr`` / ``pairs``: numpy arrays or device tensors; ``min_len`` / ``max_gap``:
    [K, NC] integers (scalars are broadcast)."""

    def __init__(self, ev_ptr, pairs, n_rec, NC, min_len, max_gap, order, out_capacity=None):
        from dcase2019_task4_amd import _lib
        self._lib, self.l = _lib, _lib.lib()
        dev = lambda a, dt: a if torch.is_tensor(a) else torch.from_numpy(np.array(a, dtype=dt, order="C")).cuda()
        self.ev_ptr = dev(ev_ptr, np.int64)
        self.pairs = dev(np.asarray(pairs).reshape(-1, 2) if not torch.is_tensor(pairs) else pairs, np.int32)
        self.n_cols, self.cap, self.n_rec, self.NC, self.order = self.ev_ptr.numel() - 1, self.pairs.shape[0], n_rec, NC, order
        K = max(self.n_cols // (n_rec * NC), 1)
        self.min_len = dev(np.broadcast_to(np.asarray(min_len, np.int32), (K, NC)), np.int32)
        self.max_gap = dev(np.broadcast_to(np.asarray(max_gap, np.int32), (K, NC)), np.int32)
        if self.cap == 0:
            self.pairs = torch.full((1, 2), SENT, dtype=torch.int32, device="cuda")              # (an address; no row is given)
        self.out_cap = self.cap if out_capacity is None else int(out_capacity)
        self.out_ptr = torch.empty(self.n_cols + 1 + TAIL, dtype=torch.int64, device="cuda")
        self.out_pairs = torch.empty(self.out_cap + TAIL, 2, dtype=torch.int32, device="cuda")
        self.err = torch.empty(2, dtype=torch.int32, device="cuda")
        self.ws_bytes = self.l.sed_events_process_ws_bytes(self.cap, self.n_cols)
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
        a = dict(cap=self.cap, n_cols=self.n_cols, n_rec=self.n_rec, NC=self.NC, ws_bytes=self.ws_bytes, ev_ptr=self.ev_ptr,
                 out_pairs=self.out_pairs, order=self.order, min_len=self.min_len, out_cap=self.out_cap)
        a.update(kw)
        return self.l.sed_events_process(p(a["ev_ptr"]), p(self.pairs), a["cap"], a["n_cols"], a["n_rec"], a["NC"], p(a["min_len"]),
                                         p(self.max_gap), a["order"], p(self.out_ptr), p(a["out_pairs"]), a["out_cap"], p(self.ws),
                                         a["ws_bytes"], p(self.err), self._lib.stream_ptr())

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


def _table(cols, pad=3):
    """Columns (lists of (on, off)) as (ev_ptr, pairs [events | pad sentinel rows])."""
    ptr = np.r_[0, np.cumsum([len(c) for c in cols])].astype(np.int64)
    rows = [e for c in cols for e in c] + [(SENT, SENT)] * pad
    return ptr, np.asarray(rows, dtype=np.int32).reshape(-1, 2)


def _check(call_out, want):
    out_ptr, out_pairs, err = call_out
    assert err == 0
    np.testing.assert_array_equal(out_ptr, want[0])
    np.testing.assert_array_equal(out_pairs[:out_ptr[-1]], want[1])
    assert (out_pairs[out_ptr[-1]:] == SENT).all()                             # nothing beyond the true count


def _columns(out_ptr, out_pairs):
    return [[tuple(int(v) for v in e) for e in out_pairs[out_ptr[c]:out_ptr[c + 1]]] for c in range(len(out_ptr) - 1)]


def _run_and_check(cols, m, g, order, pad=3, n_rec=1, NC=1):
    """The call on `cols` against the loops; returns the result's columns."""
    ptr, pairs = _table(cols, pad)
    want = ep.process_table(ptr, pairs, n_rec, NC, np.broadcast_to(m, (len(cols) // (n_rec * NC), NC)),
                            np.broadcast_to(g, (len(cols) // (n_rec * NC), NC)), order)
    _check(ProcCall(ptr, pairs, n_rec, NC, m, g, order).run(), want)
    return _columns(*want)


def _spaced(n, t0=0, step=4, length=2):
    return [(t0 + step * k, t0 + step * k + length) for k in range(n)]


# ---- 1. the entry alone, on hand-made tables --------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_zero_capacity_one_event_and_a_capacity_far_above_the_count(order):
    z = np.zeros(4, np.int64)
    out_ptr, out_pairs, err = ProcCall(z, np.zeros((0, 2), np.int32), 1, 3, 2, 2, order).run()   # no rows: the flat passes have no grid
    assert err == 0 and (out_ptr == 0).all() and out_pairs.shape[0] == 0
    out_ptr, _, err = ProcCall(z, np.full((5, 2), SENT, np.int32), 3, 1, 2, 2, order).run()      # capacity without events
    assert err == 0 and (out_ptr == 0).all()
    assert _run_and_check([[(4, 9)]], 5, 3, order, pad=0) == [[(4, 9)]]                         # one column with one event
    assert _run_and_check([[(4, 9)]], 6, 3, order, pad=0) == [[]]
    cols = [_spaced(5), [], _spaced(3, 100, 3, 1)]
    assert _run_and_check(cols, 2, 1, order, pad=3000, NC=3) == [_spaced(5), [], []]              # tail indices of no column
    assert ProcCall(*_table(cols), 1, 3, 2, 1, order).run(err0=32)[2] == 32                      # a given word is OR-ed into


@pytest.mark.parametrize("order", ORDERS)
def test_the_orders_differ_and_g_0_fuses_abutting_events_only(order):
    got = _run_and_check([[(0, 1), (2, 3), (4, 5)], [(0, 2), (2, 5), (6, 7), (7, 8), (10, 11)]], [[3, 0]], [[2, 0]], order, NC=2)
    assert got == [[] if order == 0 else [(0, 5)], [(0, 5), (6, 8), (10, 11)]]
    far = [[(-2 ** 31, -2 ** 31 + 1), (2 ** 31 - 2, 2 ** 31 - 1)], [(-2 ** 31, 2 ** 31 - 1)]]    # differences beyond 32 bits
    assert _run_and_check(far, 1, 2 ** 31 - 1, order) == far
    assert _run_and_check(far, 2 ** 31 - 1, -1, order) == [[], far[1]]


@pytest.mark.parametrize("order", ORDERS)
def test_column_edges_on_wave_and_workgroup_edges_with_empty_columns_between(order):
    """Every column restarts at time 0, so an event that took the event in front of its column's start for its predecessor
    would fuse with it (a negative gap): the columns start on index 64, on 256 and in the middle of a wave."""
    sizes = [64, 0, 192, 0, 0, 100, 156, 1, BLOCK, 3]
    cols = [_spaced(n) for n in sizes]
    ptr, _ = _table(cols)
    assert {64, BLOCK, BLOCK + 100, 2 * BLOCK, 3 * BLOCK + 1}.issubset(set(ptr.tolist()))
    got = _run_and_check(cols, 0, 2, order, NC=2)                              # every column one chain
    assert got == [[(0, 4 * n - 2)] if n else [] for n in sizes]
    _run_and_check(cols, 3, 1, order, NC=5)                                    # nothing fuses: all dropped
    _run_and_check(cols, [[0, 3]], [[2, -1]], order, NC=2)                      # alternately per class
    _run_and_check(cols, [[0, 3], [5, 0], [2, 2], [-1, 9], [1, 1]], [[2, -1], [0, 1], [2, 2], [3, 0], [9, 9]], order, NC=2)   # K = 5


@pytest.mark.parametrize("order", ORDERS)
def test_a_chain_of_600_events_across_two_workgroup_edges(order):
    n = 600
    one = [(5 * k, 5 * k + 2) for k in range(n)]                               # gaps of 3
    assert _run_and_check([one], 0, 3, order) == [[(0, 5 * n - 3)]]
    assert len(_run_and_check([one], 0, 2, order)[0]) == n
    on = np.cumsum(np.tile([5, 3], n // 2))                                    # gaps 1, 3, 1, 3 ...: every second pair fuses
    alt = [(int(a), int(a) + 2) for a in on]
    got = _run_and_check([alt], 0, 1, order)
    assert len(got[0]) == n // 2 and got[0][0] == (alt[0][0], alt[1][1])
    assert len(_run_and_check([alt], 5, 1, order)[0]) == (0 if order == 0 else n // 2)     # 2 long each, 5 long when fused
    assert len(_run_and_check([[(0, 9)] + alt[5:]], 5, 1, order)[0]) == (1 if order == 0 else 1 + len(alt[5:]) // 2)


@pytest.mark.parametrize("order", ORDERS)
def test_a_run_of_600_dropped_events_between_two_kept_ones(order):
    """Order 0: the predecessor of a kept event is the previous KEPT event of its column, 600 dropped events and two
    workgroup edges away.  (Order 1 runs the same tables against its own statement.)"""
    run = [(12 + 2 * k, 13 + 2 * k) for k in range(600)]                        # 1 frame each, the last one ends at 1211
    first, last = (0, 10), (1212, 1222)
    m = 5
    within = _run_and_check([[first] + run + [last]], m, 1202, order)
    beyond = _run_and_check([[first] + run + [last]], m, 1201, order)
    if order == 0:
        assert within == [[(0, 1222)]] and beyond == [[first, last]]
    assert _run_and_check([run + [last, (1230, 1240)]], m, 7, order) == ([[last, (1230, 1240)]] if order == 0 else [[(12, 1222), (1230, 1240)]])
    assert _run_and_check([[first] + run], m, 5000, order) == [[first] if order == 0 else [(0, 1211)]]
    # the next column begins inside the same workgroup: its kept event must not take the kept event of the column before for
    # its predecessor, nor a dropped run reach across the start
    cols = [[first] + run[:100], run[:50] + [(120, 130)], run[:30], [(0, 10), (20, 30)]]
    got = _run_and_check(cols, m, 1202, order)
    if order == 0:
        assert got == [[first], [(120, 130)], [], [(0, 30)]]
    _run_and_check([[first] + run, run, run + [last], [], [first] + run + [last], [last]], [[m, 1]], [[1202, 0]], order, NC=2)


@functools.lru_cache(maxsize=None)
def _big_table():
    """STRIP * BLOCK + 257 events in five columns (one empty): more workgroups than one strip of the scans.  Lengths 1 .. 4,
    gaps 1 .. 8, so at (2, 3) a good part is dropped and a good part fused."""
    n = STRIP * BLOCK + 257
    rs = np.random.RandomState(9)
    sizes = [100000, 0, 61000, 257, n - 161257]
    rows = []
    for s in sizes:
        length, gap = rs.randint(1, 5, size=s), rs.randint(1, 9, size=s)
        off = np.cumsum(length + gap)
        rows.append(np.stack([off - length, off], 1))
    ptr = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    pairs = np.concatenate(rows + [np.full((100, 2), SENT)]).astype(np.int32)
    return ptr, pairs


@functools.lru_cache(maxsize=None)
def _big_want(order):
    ptr, pairs = _big_table()
    return ep.process_table_fast(ptr, pairs, 1, 5, [[2, 2, 2, 0, 3]], [[3, 3, 3, 8, 1]], order)


@pytest.mark.parametrize("order", ORDERS)
def test_more_workgroups_than_a_scan_strip_twice_and_one_graph_replay(order):
    ptr, pairs = _big_table()
    want = _big_want(order)
    assert ptr[-1] == STRIP * BLOCK + 257 and pairs.nbytes > 2 << 20 and 0.2 < want[0][-1] / ptr[-1] < 0.8
    small = (ptr[:3], pairs[:ptr[2]])                                          # the fast statement is the loops
    loops = ep.process_table(*small, 1, 2, [[2, 2]], [[3, 3]], order)
    np.testing.assert_array_equal(loops[0], want[0][:3])
    np.testing.assert_array_equal(loops[1], want[1][:want[0][2]])
    call = ProcCall(ptr, pairs, 1, 5, [[2, 2, 2, 0, 3]], [[3, 3, 3, 8, 1]], order)
    first = call.run()
    _check(first, want)
    second = call.run()
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    graph = torch.cuda.CUDAGraph()
    call.fill()
    with torch.cuda.graph(graph):
        assert call.launch() == 0
    call.fill()
    graph.replay()
    replay = call.get()
    assert replay[2] == 0 and replay[0].tobytes() == first[0].tobytes() and replay[1].tobytes() == first[1].tobytes()


@pytest.mark.parametrize("order", ORDERS)
def test_one_event_too_many_raises_bit_2_and_writes_nothing_beyond(order):
    ptr, pairs = _big_table()
    want = _big_want(order)
    n = int(want[0][-1])
    out_ptr, out_pairs, err = ProcCall(ptr, pairs, 1, 5, [[2, 2, 2, 0, 3]], [[3, 3, 3, 8, 1]], order, out_capacity=n - 1).run()
    assert err == 2                                                            # (get() checked the guard-filled tail behind it)
    np.testing.assert_array_equal(out_ptr, want[0])                            # ALWAYS the true counts
    _check(ProcCall(ptr, pairs, 1, 5, [[2, 2, 2, 0, 3]], [[3, 3, 3, 8, 1]], order, out_capacity=n).run(), want)


def _err_cols():
    return [_spaced(3), [], _spaced(4, 0, 5, 1), _spaced(2, 7), _spaced(3, 1, 9, 4)]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("entry,value,skipped,undefined", [(0, -2, (0,), ()), (1, -5, (0, 1), ()), (5, 10 ** 6, (4,), ()),
                                                            (2, 2, (1,), (0, 2))])
def test_broken_offsets_raise_bit_16_and_leave_the_other_columns_right(order, entry, value, skipped, undefined):
    """A negative entry, one beyond the capacity and a decreasing one (entry 2 below entry 1: column 1 ends in front of its
    start and is skipped, column 2 has valid bounds that are not its own and reach into column 0)."""
    cols = _err_cols()
    ptr, pairs = _table(cols)
    want = _columns(*ep.process_table(ptr, pairs, 1, 1, np.full((5, 1), 2), np.full((5, 1), 2), order))
    ptr = ptr.copy()
    ptr[entry] = value
    out_ptr, out_pairs, err = ProcCall(ptr, pairs, 1, 1, 2, 2, order).run()
    assert err & 16 and not err & ~(16 | 64)
    got = _columns(out_ptr, out_pairs)
    for c in range(len(cols)):
        if c not in undefined:
            assert got[c] == ([] if c in skipped else want[c]), c


@pytest.mark.parametrize("order", ORDERS)
def test_columns_that_are_not_sorted_and_disjoint_raise_bit_64(order):
    cols = _err_cols()
    ptr, pairs = _table(cols)
    want = _columns(*ep.process_table(ptr, pairs, 1, 1, np.full((5, 1), 2), np.full((5, 1), 2), order))
    i = int(ptr[2])
    for what in ("unsorted", "overlap", "empty event"):
        bad = pairs.copy()
        if what == "unsorted":
            bad[[i, i + 1]] = bad[[i + 1, i]]
        elif what == "overlap":
            bad[i, 1] = bad[i + 1, 0] + 1
        else:
            bad[i + 3, 1] = bad[i + 3, 0]                                      # the column's last event: on == off
        out_ptr, out_pairs, err = ProcCall(ptr, bad, 1, 1, 2, 2, order).run()
        assert err == 64, what
        got = _columns(out_ptr, out_pairs)
        assert [g for c, g in enumerate(got) if c != 2] == [w for c, w in enumerate(want) if c != 2], what
    abut = pairs.copy()
    abut[i, 1] = abut[i + 1, 0]                                                # off == the next on is in order
    assert ProcCall(ptr, abut, 1, 1, 2, 2, order).run()[2] == 0


def test_bad_host_arguments_return_before_any_launch():
    call = ProcCall(*_table([_spaced(3)] * 6), 2, 3, 1, 1, 0)
    call.fill()
    l = call.l
    assert l.sed_events_process_ws_bytes(1 << 31, 4) == 0 and l.sed_events_process_ws_bytes(8, 1 << 26) == 0
    assert l.sed_events_process_ws_bytes(-1, 4) == 0 and l.sed_events_process_ws_bytes(8, 0) == 0
    bad_arg, bad_ws = -1, -2                                                   # SED_ERR_BAD_ARG, SED_ERR_WORKSPACE
    assert call.launch(ev_ptr=None) == bad_arg and b"null" in l.sed_last_error()
    assert call.launch(min_len=None) == bad_arg
    assert call.launch(cap=1 << 31) == bad_arg and call.launch(n_cols=0) == bad_arg and call.launch(out_cap=-1) == bad_arg
    assert call.launch(n_rec=4) == bad_arg and b"multiple" in l.sed_last_error()                 # 6 columns, 4 x 3 per point
    assert call.launch(NC=5) == bad_arg and call.launch(n_rec=0) == bad_arg and call.launch(NC=0) == bad_arg
    assert call.launch(order=2) == bad_arg and call.launch(order=-1) == bad_arg
    assert call.launch(out_pairs=call.pairs) == bad_arg
    assert call.launch(out_pairs=call.out_pairs.reshape(-1)[1:]) == bad_arg and b"aligned" in l.sed_last_error()
    assert call.launch(ws_bytes=call.ws_bytes + 8) == bad_ws and b"ws_bytes" in l.sed_last_error()
    assert call.launch(ws_bytes=0) == bad_ws
    torch.cuda.synchronize()
    assert (call.out_ptr == SENT).all() and (call.out_pairs == SENT).all() and int(call.err[0].item()) == 0


# ---- 2. on the tables of sed_stitch_sweep -------------------------------------------------------------------------------------------
T3_G = 16
K_G, NREC_G, NC_G = 3, 2, 3


@functools.lru_cache(maxsize=None)
def _sweep_table(lengths):
    """The table sed_stitch_sweep leaves for K_G points on two smooth recordings (windows that tile them: the blend copies)."""
    rec_win0, rec_frame0 = _tables(list(lengths), T3_G, T3_G)
    rs = np.random.RandomState(sum(lengths))
    p = rs.uniform(size=(rec_win0[-1], T3_G, NC_G)).astype(np.float32)
    tls = [smooth_timeline(40 + L, L, NC_G) for L in lengths]
    for r, L in enumerate(lengths):
        for j in range(rec_win0[r + 1] - rec_win0[r]):
            n = min(T3_G, L - j * T3_G)
            p[rec_win0[r] + j, :n] = tls[r][j * T3_G:j * T3_G + n]
    tl = np.concatenate(tls)
    thr = np.stack([np.quantile(tl, q, axis=0) for q in (0.35, 0.5, 0.65)]).astype(np.float32)
    win = np.array([[1, 1, 3], [1, 3, 1], [3, 1, 1]], np.int32)
    sweep = StitchCall(p, rec_win0, rec_frame0, T3_G, 1, thr, win, sweep=True)
    out = sweep.run()
    assert out["err"] == 0
    n_cols = K_G * NREC_G * NC_G
    counts = np.concatenate([np.diff(stitch_np.decode(tl, rec_frame0, thr[k], win[k])[1]) for k in range(K_G)])
    assert (np.diff(out["ev_ptr"]) == counts).all()                            # (the decode of the statement, K_G times)
    return sweep.ev_ptr[:n_cols + 1].clone(), sweep.ev_pairs[:sweep.capacity].clone(), out["ev_ptr"], out["ev_pairs"][:sweep.capacity]


GRID_PARAMS = [(np.array([[0, 2, 3], [4, 1, 2], [2, 2, 6]]), np.array([[1, -1, 2], [0, 3, 5], [2, 2, 1]])),
               (np.array([[3, 3, 3], [1, 5, 2], [0, 0, 9]]), np.array([[4, 0, 1], [7, 2, -1], [1, 1, 3]]))]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("lengths", [(1, 700), (2, 77)])
def test_sweep_tables_with_parameters_per_point_and_class(lengths, order):
    d_ptr, d_pairs, ptr, pairs = _sweep_table(lengths)
    n_cols, per_point = K_G * NREC_G * NC_G, NREC_G * NC_G
    assert ptr[-1] > (40 if max(lengths) == 700 else 4)
    for min_len, max_gap in GRID_PARAMS:
        want = ep.process_table(ptr, pairs, NREC_G, NC_G, min_len, max_gap, order)
        got = ProcCall(d_ptr, d_pairs, NREC_G, NC_G, min_len, max_gap, order).run()
        _check(got, want)
        # the K-point call is K one-point calls, byte for byte
        ptrs, rows = [np.zeros(1, np.int64)], []
        for k in range(K_G):
            one = ProcCall(d_ptr[k * per_point:(k + 1) * per_point + 1], d_pairs, NREC_G, NC_G, min_len[k:k + 1], max_gap[k:k + 1],
                           order).run()
            assert one[2] == 0 and one[0][0] == 0
            ptrs.append(one[0][1:] + ptrs[-1][-1])
            rows.append(one[1][:one[0][-1]])
        assert np.concatenate(ptrs).tobytes() == got[0].tobytes()
        assert np.concatenate(rows).tobytes() == got[1][:got[0][-1]].tobytes()
        # applying the call to its own output changes nothing
        n = int(got[0][-1])
        again = ProcCall(got[0], got[1][:max(n, 1)] if n else np.zeros((0, 2), np.int32), NREC_G, NC_G, min_len, max_gap, order).run()
        assert again[2] == 0 and again[0].tobytes() == got[0].tobytes() and again[1][:n].tobytes() == got[1][:n].tobytes()
    # the identity: min_len <= 0 and max_gap < 0 return the input's bytes
    same = ProcCall(d_ptr, d_pairs, NREC_G, NC_G, np.array([[0, -1, 0]] * K_G), np.array([[-1, -1, -9]] * K_G), order).run()
    assert same[2] == 0 and same[0].tobytes() == ptr.tobytes() and same[1][:ptr[-1]].tobytes() == pairs[:ptr[-1]].tobytes()


def test_the_python_entry_takes_host_and_device_parameters_and_ors_into_a_given_word():
    from dcase2019_task4_amd.inference import events_process
    d_ptr, d_pairs, ptr, pairs = _sweep_table((1, 700))
    min_len, max_gap = GRID_PARAMS[0]
    for order, code in (("drop_merge", 0), ("merge_drop", 1)):
        want = ep.process_table(ptr, pairs, NREC_G, NC_G, min_len, max_gap, code)
        out_ptr, out_pairs, err = events_process(d_ptr, d_pairs, NREC_G, NC_G, min_len, max_gap, order)
        assert int(err.item()) == 0 and out_pairs.shape[0] == d_pairs.shape[0]
        np.testing.assert_array_equal(out_ptr.cpu().numpy(), want[0])
        np.testing.assert_array_equal(out_pairs.cpu().numpy()[:want[0][-1]], want[1])
        dev = lambda a: torch.from_numpy(a.astype(np.int32)).cuda()
        word = torch.full((1,), 8, dtype=torch.int32, device="cuda")
        out_ptr2, out_pairs2, err2 = events_process(d_ptr, d_pairs, NREC_G, NC_G, dev(min_len), dev(max_gap), order,
                                                    capacity=int(want[0][-1]) - 1, err=word)
        assert err2 is word and int(word.item()) == 8 | 2 and out_pairs2.shape[0] == want[0][-1] - 1
        assert torch.equal(out_ptr2, out_ptr)
    with pytest.raises(ValueError):
        events_process(d_ptr, d_pairs, NREC_G, NC_G, min_len[:2], max_gap, "drop_merge")
    with pytest.raises(ValueError):
        events_process(d_ptr, d_pairs, 4, NC_G, min_len, max_gap)


# ---- 3. through get_long_predictions and validate_long ------------------------------------------------------------------------------
def _seconds_columns(ev_ptr, ev_pairs, n_rec, NC, k=0):
    return [[[(int(a) * NUM / DEN, int(b) * NUM / DEN) for a, b in ev_pairs[ev_ptr[(k * n_rec + r) * NC + c]:ev_ptr[(k * n_rec + r) * NC + c + 1]]]
             for c in range(NC)] for r in range(n_rec)]


def test_get_long_predictions_and_validate_long_with_minimum_lengths_and_gaps():
    from dcase2019_task4_amd import metrics as M
    from dcase2019_task4_amd.inference import LongRecordingSet, get_long_predictions, process_points
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
    fs = NUM / DEN                                                             # seconds per label frame
    thr = np.stack([np.quantile(tl, q, axis=0) for q in (0.45, 0.45, 0.6)]).astype(np.float32)   # points 0 and 1 share a decode
    thr_hi = np.stack([np.quantile(tl, q, axis=0) for q in (0.7, 0.8, 0.75)]).astype(np.float32)
    win = np.array([[1] * 10, [1] * 10, [3, 1, 5, 3, 3, 1, 3, 1, 3, 1]], np.int32)
    lengths = [0.25, [2 * fs] * 5 + [4 * fs] * 5, 0.0]                          # seconds: 3 frames; 2 / 4 frames; off
    gaps = [0.15, 0.0, [3 * fs + 0.01] * 10]                                    # seconds: 1 frame; abutting only; 3 frames
    min_len, max_gap = process_points(lengths, gaps, NC, fs, K)
    assert min_len.tolist() == [[3] * 10, [2] * 5 + [4] * 5, [0] * 10] and max_gap.tolist() == [[1] * 10, [0] * 10, [3] * 10]
    pack = lambda c: M.RefEvents(*ls.pack(c), names, labels)
    plain_tables = [stitch_np.decode(tl, f0, thr[k], win[k])[1:] for k in range(K)]
    ptr0 = np.concatenate([[0]] + [t[0][1:] + sum(int(u[0][-1]) for u in plain_tables[:k]) for k, t in enumerate(plain_tables)])
    pairs0 = np.concatenate([t[1] for t in plain_tables])
    hyst_table = hy.decode_pairs(tl, f0, thr, thr_hi, win)
    ref = None
    for order, code in (("drop_merge", 0), ("merge_drop", 1)):
        want_ptr, want_pairs = ep.process_table(ptr0, pairs0, n_rec, NC, min_len, max_gap, code)
        assert 0 < want_ptr[-1] < ptr0[-1]
        cols = [_seconds_columns(want_ptr, want_pairs, n_rec, NC, k) for k in range(K)]
        if ref is None:
            ref = pack(ls.sorted_jittered_references(cols[0], 6))
        ests = [pack(c) for c in cols]
        c_w = M.long_sweep_event_counts_from_events(ests, ref)
        e_w = M.long_sweep_error_from_events(ests, ref)
        p_w = M.long_sweep_psds_counts_from_events(ests, ref)
        want = M._metric_pairs(labels, *c_w.host(), e_w.host())
        cap = lset.capacity(NC)
        for kw in (dict(), dict(max_table_bytes=8 * cap), dict(one_blend=False)):              # one chunk; a point per chunk; per point
            psds = M.PSDSCounts(K, NC, "cuda")
            got = M.validate_long(model, lset, ref, list(thr), list(win), batch_size=8, psds=psds, error_rate=True,
                                  min_event_lengths=lengths, min_event_gaps=gaps, process_order=order, **kw)
            for k in range(K):
                for i in (0, 1):
                    assert got[k][i].class_wise == want[k][i].class_wise and got[k][i].overall_sdi == want[k][i].overall_sdi, (kw, k, i)
                assert got[k][1].Ntn == want[k][1].Ntn
            assert psds.host().tobytes() == p_w.host().tobytes()
        # with a high threshold, PSDS and the error rate in the same call: hysteresis, then the statement
        h_ptr, h_pairs = ep.process_table(*hyst_table, n_rec, NC, min_len, max_gap, code)
        assert 0 < h_ptr[-1] < hyst_table[0][-1]
        h_cols = [_seconds_columns(h_ptr, h_pairs, n_rec, NC, k) for k in range(K)]
        h_ests = [pack(c) for c in h_cols]
        h_want = M._metric_pairs(labels, *M.long_sweep_event_counts_from_events(h_ests, ref).host(),
                                 M.long_sweep_error_from_events(h_ests, ref).host())
        psds = M.PSDSCounts(K, NC, "cuda")
        got = M.validate_long(model, lset, ref, list(thr), list(win), batch_size=8, psds=psds, error_rate=True,
                              thresholds_high=list(thr_hi), min_event_lengths=lengths, min_event_gaps=gaps, process_order=order)
        for k in range(K):
            for i in (0, 1):
                assert got[k][i].class_wise == h_want[k][i].class_wise and got[k][i].overall_sdi == h_want[k][i].overall_sdi, (k, i)
        assert psds.host().tobytes() == M.long_sweep_psds_counts_from_events(h_ests, ref).host().tobytes()
        # get_long_predictions: the DataFrame of the statement, per point (seconds in, one value or one per class)
        for k in range(K):
            df = get_long_predictions(model, lset, labels, batch_size=8, threshold=thr[k], median_window=win[k],
                                      min_event_length=lengths[k], min_event_gap=gaps[k], process_order=order)
            rows = df[["event_label", "onset", "offset", "filename"]].itertuples(index=False)
            assert se.columns_from_rows(rows, names, labels) == cols[k], (order, k)
            df = get_long_predictions(model, lset, labels, batch_size=8, threshold=thr[k], median_window=win[k],
                                      threshold_high=thr_hi[k], min_event_length=lengths[k], min_event_gap=gaps[k], process_order=order)
            rows = df[["event_label", "onset", "offset", "filename"]].itertuples(index=False)
            assert se.columns_from_rows(rows, names, labels) == h_cols[k], (order, k)
    # nothing asked for: today's frame and today's integers; a step that is switched off in seconds is the identity
    assert get_long_predictions(model, lset, labels, batch_size=8, min_event_length=None, min_event_gap=None).equals(plain)
    assert get_long_predictions(model, lset, labels, batch_size=8, min_event_length=0.0).equals(plain)
    base = M.validate_long(model, lset, ref, list(thr), list(win), batch_size=8)
    off = M.validate_long(model, lset, ref, list(thr), list(win), batch_size=8, min_event_lengths=[0.0], process_order="merge_drop")
    assert all(base[k][i].class_wise == off[k][i].class_wise for k in range(K) for i in (0, 1))
    with pytest.raises(ValueError, match="order"):
        M.validate_long(model, lset, ref, list(thr), list(win), min_event_gaps=[0.1], process_order="drop")
    with pytest.raises(ValueError, match="min_event_lengths"):
        M.validate_long(model, lset, ref, list(thr), list(win), min_event_lengths=[0.1, 0.2])
    with pytest.raises(ValueError, match="min_event_gaps"):
        get_long_predictions(model, lset, labels, min_event_gap=-0.1)

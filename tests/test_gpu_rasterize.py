"""-m gpu tests of sed_events_rasterize against the plain-loop statement (tests/rasterize_np.py) and of the Python built on
it: shapes and alignments, recording boundaries on the workgroup edge, permuted destinations with gaps, value bits, the
maximum over old contents, an empty table, more than 1 024 workgroups with two calls and one graph replay, the error bits,
the agreement with the stitched decode and the event scores, relabel on both kinds of set, get_long_predictions'
return_table, pseudo_label, and one epoch of training on a set relabelled in place.

Every destination starts as 0xFFFFFFFF words (NaN) or prescribed old contents, lies between a head and a tail of sentinel
words, and is compared bit for bit: there is no arithmetic in the operator, so there is no tolerance."""
import functools

import numpy as np
import pytest
import torch

from tests import gpu_util as gu
from tests import rasterize_np as rn
from tests.long_util import SENT, TAIL, _Scaler
from tests.test_event_scores_cpu import HYST_GRID, hysteresis_case

pytestmark = pytest.mark.gpu

BLOCK = 256                                                                    # timeline rows per workgroup of the row pass
FILL = 0xFFFFFFFF


def _dev(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


class RasCall:
    """One sed_events_rasterize call.  ``dst`` [dst_rows, NC] starts as ``old`` (default: 0xFFFFFFFF words) between HEAD and
    TAIL words of 0xFFFFFFFF that ``get()`` checks; ``misalign`` shifts it one float off 16-byte alignment."""
    HEAD = 4

    def __init__(self, ptr, pairs, f0, NC, dst_rows=None, row0=None, value=None, point=None, K=1, combine=0, misalign=False,
                 old=None):
        from dcase2019_task4_amd import _lib
        self._lib, self.l, self.NC, self.K, self.combine = _lib, _lib.lib(), NC, K, combine
        self.h_ptr, self.h_f0 = np.asarray(ptr, np.int64), np.asarray(f0, np.int64)
        self.h_pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        self.h_row0, self.h_value, self.h_point = row0, value, point
        self.n_rec, self.cap = len(self.h_f0) - 1, self.h_pairs.shape[0]
        self.rows = int(self.h_f0[-1]) if dst_rows is None else int(dst_rows)
        self.ptr, self.f0 = _dev(self.h_ptr, np.int64), _dev(self.h_f0, np.int64)
        self.pairs = _dev(self.h_pairs, np.int32) if self.cap else torch.full((1, 2), SENT, dtype=torch.int32, device="cuda")
        self.value = None if value is None else (_dev(value, np.float32) if self.cap else torch.zeros(1, device="cuda"))
        self.point, self.row0 = _dev(point, np.int32), _dev(row0, np.int64)
        self.old = (np.full((self.rows, NC), FILL, np.uint32).view(np.float32) if old is None
                    else np.ascontiguousarray(old, np.float32).reshape(self.rows, NC))
        head = self.HEAD + (1 if misalign else 0)
        self.buf = torch.empty(head + self.rows * NC + TAIL, dtype=torch.int32, device="cuda")
        self.dst = self.buf[head:head + self.rows * NC].view(torch.float32)
        assert self.rows == 0 or (self.dst.data_ptr() % 16 != 0) == bool(misalign)
        self.head = head
        self.err = torch.empty(2, dtype=torch.int32, device="cuda")

    def fill(self, err0=0):
        self.buf.fill_(-1)                                                     # 0xFFFFFFFF
        self.dst.view(torch.int32).copy_(torch.from_numpy(self.old.view(np.int32).reshape(-1)))
        self.err.fill_(SENT)
        self.err[:1].fill_(err0)

    def launch(self, **kw):
        p = self._lib.ptr
        a = dict(ptr=self.ptr, pairs=self.pairs, value=self.value, cap=self.cap, K=self.K, point=self.point, f0=self.f0,
                 n_rec=self.n_rec, NC=self.NC, dst=self.dst, rows=self.rows, row0=self.row0, combine=self.combine, err=self.err)
        a.update(kw)
        return self.l.sed_events_rasterize(p(a["ptr"]), p(a["pairs"]), p(a["value"]), a["cap"], a["K"], p(a["point"]), p(a["f0"]),
                                           a["n_rec"], a["NC"], p(a["dst"]), a["rows"], p(a["row0"]), a["combine"], p(a["err"]),
                                           self._lib.stream_ptr())

    def get(self):
        torch.cuda.synchronize()
        buf = self.buf.cpu().numpy().view(np.uint32)
        n = self.rows * self.NC
        assert (buf[:self.head] == FILL).all() and (buf[self.head + n:] == FILL).all() and int(self.err[1].item()) == SENT
        return buf[self.head:self.head + n].view(np.float32).reshape(self.rows, self.NC).copy(), int(self.err[0].item())

    def run(self, err0=0, **kw):
        self.fill(err0)
        assert self.launch(**kw) == 0, self.l.sed_last_error()
        return self.get()

    def want(self):
        return rn.rasterize(self.h_ptr, self.h_pairs, self.h_f0, self.n_rec, self.NC, self.old, self.h_row0, self.h_value,
                            self.h_point, self.combine, self.K)

    def check(self, err=0):
        """The call against the statement: the error word, every specified element bit for bit; returns the rows."""
        got, e = self.run()
        want, werr, unspec = self.want()
        assert e == werr == err, (e, werr, err)
        np.testing.assert_array_equal(got.view(np.uint32)[~unspec], want.view(np.uint32)[~unspec])
        return got


def _patterns(L3):
    """The column kinds of case 1 for a recording of L3 rows."""
    return [[(0, min(2, L3))] + ([(5, 6)] if L3 > 6 else []),                  # an event at row 0
            [(max(0, L3 - 3), L3)],                                            # an event ending at L3
            [(u, u + 1) for u in (1, 4, 9) if u < L3],                         # one-row events
            [e for e in ((2, 5), (5, 9), (9, 10)) if e[1] <= L3],              # touching events
            [],                                                                # an empty column
            [(0, L3)],                                                         # one event over the whole recording
            [(2 * i, 2 * i + 1) for i in range((L3 + 1) // 2)]]                # ceil(L3 / 2) one-row events


def _shape_table(NC, n_rec, K, shift, L3s):
    cols = [_patterns(L3s[(col // NC) % n_rec])[(col + shift + col // NC) % 7] for col in range(K * n_rec * NC)]
    return rn.table(cols, pad=3)


# ---- 1. shapes, alignments, column kinds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NC,n_rec,K", [(1, 1, 1), (3, 3, 3), (4, 1, 3), (4, 3, 1), (10, 3, 1), (16, 2, 3)])
def test_shapes_points_and_column_kinds_against_the_statement(NC, n_rec, K):
    L3s = [37, 300, 64][:n_rec]
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    point = [(2 * c + 1) % K for c in range(NC)]
    assert K == 1 or len(set(point)) > 1                                       # per-class points differ
    rs = np.random.RandomState(NC + n_rec + K)
    seen = set()
    for shift in range(7):
        ptr, pairs = _shape_table(NC, n_rec, K, shift, L3s)
        seen |= {(col + shift + col // NC) % 7 for col in range(K * n_rec * NC) if col // (n_rec * NC) == point[col % NC]}
        value = rs.uniform(0.1, 1, size=len(pairs)).astype(np.float32) if shift % 2 else None
        for misalign in ((False, True) if NC % 4 == 0 else (False,)):
            got = RasCall(ptr, pairs, f0, NC, value=value, point=point, K=K, misalign=misalign).check()
            assert not np.isnan(got).any()                                     # replace writes every element
        if K == 1:
            rn.same_bits(RasCall(ptr, pairs, f0, NC, value=value).check(), got)          # point NULL = all zero
    assert seen == set(range(7))


# ---- 2. recording boundaries on the workgroup edge ------------------------------------------------------------------------------------
def test_recording_boundaries_and_events_on_the_workgroup_edge():
    assert BLOCK == 256
    NC = 2
    f0 = np.array([0, 255, 256, 257, 600], np.int64)                           # boundaries at the flat rows 255, 256, 257
    cols = [[(250, 255)], [(0, 255)], [(0, 1)], [], [], [(0, 1)], [(0, 5), (300, 343)], [(342, 343)]]
    ptr, pairs = rn.table(cols, pad=2)
    RasCall(ptr, pairs, f0, NC).check()
    # one recording: an event that ends exactly on the edge, one that starts on it, one that lies across it
    cols = [[(200, 256), (256, 300)], [(255, 257), (511, 513)]]
    for L3 in (255, 256, 257, 600):
        mine = [[e for e in c if e[1] <= L3] for c in cols]
        ptr, pairs = rn.table(mine)
        got = RasCall(ptr, pairs, [0, L3], NC).check()
        assert got[:, 0].sum() == sum(off - on for on, off in mine[0])


# ---- 3. destinations ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NC", [3, 4])
def test_a_permuted_dst_row0_with_gaps_keeps_the_gaps_and_null_is_the_contiguous_map(NC):
    L3s = [37, 300, 64]
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    ptr, pairs = _shape_table(NC, 3, 1, 2, L3s)
    row0 = [430, 50, 360]
    got = RasCall(ptr, pairs, f0, NC, dst_rows=480, row0=row0).check()
    bits = got.view(np.uint32)
    for lo, hi in ((0, 50), (350, 360), (424, 430), (467, 480)):
        assert (bits[lo:hi] == FILL).all()
    flat = RasCall(ptr, pairs, f0, NC).check()
    for r in range(3):
        rn.same_bits(got[row0[r]:row0[r] + L3s[r]], flat[f0[r]:f0[r + 1]])
    rn.same_bits(RasCall(ptr, pairs, f0, NC, row0=f0[:-1]).check(), flat)


# ---- 4. values ------------------------------------------------------------------------------------------------------------------------
def test_values_are_copied_bit_for_bit_and_null_is_one():
    NC, L3 = 4, 40
    cols = [[(0, 3), (10, 12)], [(5, 6)], [(0, 40)], [(7, 9), (9, 20)]]
    ptr, pairs = rn.table(cols)
    ones = RasCall(ptr, pairs, [0, L3], NC).check()
    assert set(ones.view(np.uint32).reshape(-1).tolist()) == {0, 0x3F800000}
    value = np.array([0x7FC12345, 0x80000000, 0x00000001, 0xFF800001, 0x3F000000, 0xBF800000], np.uint32).view(np.float32)
    for misalign in (False, True):
        got = RasCall(ptr, pairs, [0, L3], NC, value=value, misalign=misalign).check().view(np.uint32)
        assert got[0, 0] == 0x7FC12345 and got[11, 0] == 0x80000000 and got[5, 1] == 1 and (got[:, 2] == 0xFF800001).all()
        assert got[8, 3] == 0x3F000000 and got[9, 3] == 0xBF800000 and got[20, 3] == 0


@pytest.mark.parametrize("NC,misalign", [(1, False), (4, False), (4, True)])
def test_the_maximum_over_old_contents(NC, misalign):
    L3 = 48
    rs = np.random.RandomState(5)
    old = rs.choice(np.array([2.0, 0.25, 0.5, np.nan, -1.0, 0.0], np.float32), size=(L3, NC)).astype(np.float32)
    cols = [[(0, 20), (24, 40)], [(3, 48)], [], [(1, 2), (2, 3), (40, 47)]][:NC]
    ptr, pairs = rn.table(cols)
    value = np.full(len(pairs), 0.5, np.float32)
    got = RasCall(ptr, pairs, [0, L3], NC, value=value, combine=1, misalign=misalign, old=old).check()
    covered = np.zeros((L3, NC), bool)
    for c, col in enumerate(cols):
        for on, off in col:
            covered[on:off, c] = True
    rn.same_bits(got[~covered], old[~covered])                                 # uncovered elements stay, NaN included
    for v, w in ((2.0, 2.0), (0.25, 0.5), (0.5, 0.5), (-1.0, 0.5), (0.0, 0.5)):
        assert (got[covered & (old == np.float32(v))] == np.float32(w)).all()
    assert np.isnan(got[covered & np.isnan(old)]).all() and (covered & np.isnan(old)).any()
    nan_value = np.full(len(pairs), np.nan, np.float32)
    rn.same_bits(RasCall(ptr, pairs, [0, L3], NC, value=nan_value, combine=1, misalign=misalign, old=old).check(), old)
    # two tables by two calls are the union
    first = RasCall(ptr, pairs, [0, L3], NC, old=np.zeros((L3, NC), np.float32)).check()
    other = rn.table([[(18, 30)], [(0, 1)], [(4, 6)], []][:NC])
    both = RasCall(*other, [0, L3], NC, combine=1, old=first).check()
    covered[18:30, 0] = True
    if NC > 1:
        covered[0:1, 1] = True
        covered[4:6, 2] = True
    rn.same_bits(both, covered.astype(np.float32))


# ---- 5. an empty table ----------------------------------------------------------------------------------------------------------------
def test_an_empty_table_with_no_capacity():
    NC, f0 = 4, [0, 30, 70]
    ptr, pairs = np.zeros(2 * NC + 1, np.int64), np.zeros((0, 2), np.int32)
    call = RasCall(ptr, pairs, f0, NC)
    assert call.cap == 0
    got = call.check()
    assert (got.view(np.uint32) == 0).all()                                    # +0.0f everywhere
    old = np.random.RandomState(0).standard_normal((70, NC)).astype(np.float32)
    rn.same_bits(RasCall(ptr, pairs, f0, NC, combine=1, old=old).check(), old)
    none = RasCall(ptr[:NC + 1], pairs, [0, 0], NC, dst_rows=0)                # no rows: the check pass alone
    got, err = none.run(dst=none.buf)
    assert err == 0 and got.size == 0


# ---- 6. more than 1 024 workgroups, two calls, one graph replay -------------------------------------------------------------------------
def test_more_than_1024_workgroups_twice_and_one_graph_replay():
    NC, L3 = 4, 1024 * BLOCK + 700
    rs = np.random.RandomState(2)
    cols = []
    for c in range(NC):
        if c == 2:
            cols.append([])
            continue
        on = np.cumsum(rs.randint(1, 9, size=L3 // 6))
        length = rs.randint(1, 4, size=on.size)
        off = np.minimum(on + length, np.r_[on[1:], L3])
        keep = (on < L3) & (off <= L3)
        cols.append(list(zip(on[keep].tolist(), off[keep].tolist())))
    ptr, pairs = rn.table(cols, pad=5)
    value = rs.uniform(0.1, 1, size=len(pairs)).astype(np.float32)
    call = RasCall(ptr, pairs, [0, L3], NC, value=value)
    assert -(-L3 // BLOCK) > 1024 and ptr[-1] > 100000
    eager = call.check()
    again, err = call.run()
    assert err == 0 and again.tobytes() == eager.tobytes()
    graph = torch.cuda.CUDAGraph()
    call.fill()
    with torch.cuda.graph(graph):
        assert call.launch() == 0
    call.fill()
    graph.replay()
    replay, err = call.get()
    assert err == 0 and replay.tobytes() == eager.tobytes()


# ---- 7. the error bits ----------------------------------------------------------------------------------------------------------------
def _err_case():
    NC, L3s = 2, [300, 40, 500]
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    cols = [[(0, 3), (5, 40), (200, 300)], [(1, 2)], [(0, 40)], [(2, 9), (10, 30)], [(4, 5), (100, 140)], [(0, 500)]]
    return f0, NC, cols


@pytest.mark.parametrize("entry,value", [(0, -2), (1, -5), (6, 10 ** 6), (3, 2)])
def test_broken_column_bounds_raise_bit_16_and_leave_the_rest_right(entry, value):
    f0, NC, cols = _err_case()
    ptr, pairs = rn.table(cols, pad=2)
    bad = ptr.copy()
    bad[entry] = value                                                         # negative, beyond the capacity, decreasing
    call = RasCall(bad, pairs, f0, NC)
    got, err = call.run()
    want, werr, unspec = call.want()
    assert err == werr and err & 16 and not err & ~(16 | 64)
    np.testing.assert_array_equal(got.view(np.uint32)[~unspec], want.view(np.uint32)[~unspec])
    assert (got.view(np.uint32) == FILL).any() and (got.view(np.uint32) != FILL).any()


@pytest.mark.parametrize("entry,value", [(3, 10 ** 6), (0, -1), (2, 290), (1, 10 ** 6)])
def test_broken_rec_frame0_raises_bit_16_and_leaves_the_other_recordings_right(entry, value):
    f0, NC, cols = _err_case()
    ptr, pairs = rn.table(cols)
    ok = RasCall(ptr, pairs, f0, NC).check()
    bad = f0.copy()
    bad[entry] = value
    call = RasCall(ptr, pairs, bad, NC, dst_rows=int(f0[-1]))
    got, err = call.run()
    assert err & 16 and not err & ~(16 | 64)
    if entry == 2:                  # recording 1 runs backwards and recording 2 starts inside recording 0: the rows in front are 0's
        rn.same_bits(got[:290], ok[:290])
        return
    broken_rows = np.ones(len(got), bool)
    for r in range(3):
        a, b = int(bad[r]), int(bad[r + 1])
        if 0 <= a <= b <= f0[-1]:
            assert (a, b) == (int(f0[r]), int(f0[r + 1]))
            rn.same_bits(got[a:b], ok[a:b])
            broken_rows[a:b] = False
    assert (got.view(np.uint32)[broken_rows] == FILL).all() and broken_rows.any()      # nothing of a broken recording is written


@pytest.mark.parametrize("row0", [[-1, 300, 340], [0, 300, 341], [0, 2 ** 40, 340]])
def test_dst_row0_outside_the_rows_raises_bit_16_and_leaves_the_other_recordings_right(row0):
    f0, NC, cols = _err_case()
    ptr, pairs = rn.table(cols)
    ok = RasCall(ptr, pairs, f0, NC).check()
    got = RasCall(ptr, pairs, f0, NC, row0=row0).check(err=16)
    bad = [r for r in range(3) if row0[r] != f0[r]]
    for r in range(3):
        if r in bad:
            assert (got.view(np.uint32)[f0[r]:f0[r + 1]] == FILL).all()
        else:
            rn.same_bits(got[f0[r]:f0[r + 1]], ok[f0[r]:f0[r + 1]])


@pytest.mark.parametrize("event", [(7, 7), (9, 3), (-1, 4), "L3", "overlap", "unsorted"])
def test_bad_events_raise_bit_64_and_leave_the_other_columns_right(event):
    NC, L3s = 2, [1300, 40]
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    dense = [(2 * i, 2 * i + 1) for i in range(600)]                           # a long column: bad events far from any row's find
    cols = [list(dense), [(1, 2), (50, 60)], [(0, 40)], [(2, 9), (10, 30)]]
    if event == "L3":
        cols[0][-1] = (L3s[0] - 1, L3s[0] + 1)
    elif event == "overlap":
        cols[0][300], cols[0][301] = (600, 603), (602, 604)
    elif event == "unsorted":
        cols[0][300], cols[0][301] = cols[0][301], cols[0][300]
    else:
        cols[0][300] = event
    ptr, pairs = rn.table(cols, pad=1)
    call = RasCall(ptr, pairs, f0, NC)
    got = call.check(err=64)
    _, _, unspec = call.want()
    assert unspec[:1300, 0].all() and unspec.sum() == 1300
    assert not np.isnan(got[:, 1]).any() and not np.isnan(got[1300:, 0]).any()
    cols[0] = dense                                                            # the same table, sound: no bit
    RasCall(*rn.table(cols, pad=1), f0, NC).check()


@pytest.mark.parametrize("bad_point", [-1, 3])
def test_a_point_outside_the_table_raises_bit_8_and_keeps_that_class(bad_point):
    NC, n_rec, K, L3s = 4, 2, 3, [37, 64]
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    ptr, pairs = _shape_table(NC, n_rec, K, 1, L3s)
    for misalign in (False, True):
        got = RasCall(ptr, pairs, f0, NC, point=[1, bad_point, 0, 2], K=K, misalign=misalign).check(err=8).view(np.uint32)
        assert (got[:, 1] == FILL).all() and not (got[:, [0, 2, 3]] == FILL).any()


def test_bad_host_arguments_return_before_any_launch():
    f0, NC, cols = _err_case()
    ptr, pairs = rn.table(cols)
    call = RasCall(ptr, pairs, f0, NC, value=np.ones(len(pairs), np.float32), point=[0, 0], row0=f0[:-1])
    call.fill(err0=5)
    l = call.l
    for name in ("ptr", "pairs", "f0", "dst", "err"):
        assert call.launch(**{name: None}) != 0 and b"null" in l.sed_last_error(), name
    for kw in (dict(NC=17), dict(NC=0), dict(n_rec=0), dict(K=0), dict(K=4097), dict(cap=1 << 31), dict(cap=-1),
               dict(rows=(1 << 31) // NC), dict(rows=-1), dict(combine=2)):
        assert call.launch(**kw) != 0, kw
    for name in ("ptr", "pairs", "value", "point", "f0", "row0"):
        assert call.launch(dst=getattr(call, name)) != 0 and b"overlaps" in l.sed_last_error(), name
    torch.cuda.synchronize()
    assert (call.buf.cpu().numpy().view(np.uint32) == FILL).all() and call.err.tolist() == [5, SENT]


# ---- 8 - 10. agreement with the existing code -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("NC,hop3,weighting", HYST_GRID)
def test_the_rasterised_decode_is_the_binary_timeline_of_the_decode(NC, hop3, weighting):
    from dcase2019_task4_amd.inference import rasterize_decoded, stitch_decode
    p, rec_win0, rec_frame0, tl, thr_lo, thr_hi = hysteresis_case(NC, hop3, weighting)
    n_rec = len(rec_frame0) - 1
    dev = lambda a: torch.from_numpy(a).cuda()
    d_f0 = dev(rec_frame0)
    for win, want_timeline in ((1, False), (5, True)):
        out = stitch_decode(dev(p), dev(rec_win0), d_f0, int(rec_frame0[-1]), hop3, thr_lo[1], win, ("uniform", "taper")[weighting],
                            want_timeline=want_timeline, want_binary=True)
        ras = rasterize_decoded(out, d_f0, n_rec, NC)
        assert int(ras["err"].item()) == 0 and ras["err"] is out["err"] and ras["ev_ptr"] is out["ev_ptr"]
        binary = out["binary"].cpu().numpy()
        assert 0.2 < binary.mean() < 0.8
        rn.same_bits(ras["labels"].cpu().numpy(), binary.astype(np.float32))
    with pytest.raises(ValueError, match="timeline"):
        rasterize_decoded(dict(out, timeline=None), d_f0, n_rec, NC, soft="max")
    soft = rasterize_decoded(out, d_f0, n_rec, NC, soft="max")
    labels = soft["labels"].cpu().numpy()
    assert int(soft["err"].item()) == 0 and ((labels > 0) == (binary > 0)).all() and labels.max() <= tl.max()


def _clip_tables(n, T, NC, seed):
    """Random tables without touching events for n clips of T rows: columns, the table, the device tables."""
    rs = np.random.RandomState(seed)
    cols = []
    for _ in range(n * NC):
        edges = np.sort(rs.choice(np.arange(0, T + 1), size=2 * rs.randint(0, 6), replace=False))
        col = [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]
        cols.append([e for i, e in enumerate(col) if i == 0 or e[0] > col[i - 1][1]])
    ptr, pairs = rn.table(cols, pad=2)
    f0 = np.arange(n + 1, dtype=np.int64) * T
    return cols, ptr, pairs, f0


def test_decoding_rasterised_clips_returns_the_table_and_their_scores_are_one():
    from dcase2019_task4_amd.inference import events_rasterize, events_scores, stitch_decode
    n, T, NC = 5, 157, 4
    cols, ptr, pairs, f0 = _clip_tables(n, T, NC, 4)
    assert ptr[-1] > 30
    d_ptr, d_pairs, d_f0 = torch.from_numpy(ptr).cuda(), torch.from_numpy(pairs).cuda(), torch.from_numpy(f0).cuda()
    labels, err = events_rasterize((d_ptr, d_pairs), d_f0, n, NC)
    assert int(err.item()) == 0 and labels.shape == (n * T, NC)
    want, werr, _ = rn.rasterize(ptr, pairs, f0, n, NC, np.zeros((n * T, NC), np.float32))
    rn.same_bits(labels.cpu().numpy(), want)
    rec_win0 = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    back = stitch_decode(labels.reshape(n, T, NC), rec_win0, d_f0, n * T, T, threshold=0.5, median_window=1)
    assert int(back["err"].item()) == 0
    m = int(ptr[-1])
    assert back["ev_ptr"].cpu().numpy().tobytes() == ptr.tobytes()
    assert back["ev_pairs"].cpu().numpy()[:m].tobytes() == pairs[:m].tobytes()
    smax, smean, err = events_scores((d_ptr, d_pairs), labels, d_f0, n, NC)
    one = np.ones(m, np.float32)
    assert int(err.item()) == 0
    rn.same_bits(smax.cpu().numpy()[:m], one)
    rn.same_bits(smean.cpu().numpy()[:m], one)
    # the thin call's other arguments: a given destination and word, points, values, combine
    K2 = torch.cat([d_ptr, d_ptr[1:] + d_ptr[-1]])
    pairs2 = torch.cat([d_pairs[:m], d_pairs[:m]])
    word = torch.full((1,), 32, dtype=torch.int32, device="cuda")
    dst = torch.full((n * T + 3, NC), 0.25, device="cuda")
    vals = torch.full((2 * m,), 0.5, device="cuda")
    vals[m:] = 0.75
    out, got_word = events_rasterize({"ev_ptr": K2, "ev_pairs": pairs2}, d_f0, n, NC, dst=dst, values=vals, point=[0, 1, 1, 0],
                                     combine="max", err=word)
    assert out is dst and got_word is word and int(word.item()) == 32
    h = dst.cpu().numpy()
    assert (h[n * T:] == 0.25).all()
    for c, v in enumerate((0.5, 0.75, 0.75, 0.5)):
        np.testing.assert_array_equal(h[:n * T, c], np.where(want[:, c] > 0, np.float32(v), np.float32(0.25)))
    with pytest.raises(ValueError, match="combine"):
        events_rasterize((d_ptr, d_pairs), d_f0, n, NC, combine="sum")
    with pytest.raises(ValueError, match="point"):
        events_rasterize((d_ptr, d_pairs), d_f0, n, NC, point=1)
    with pytest.raises(ValueError, match="overlap"):
        events_rasterize((d_ptr, d_pairs), d_f0, n, NC, dst=dst, dst_row0=[0, T, 2 * T - 1, 3 * T, 4 * T], rec_frame0_host=f0)


# ---- 11. relabel ----------------------------------------------------------------------------------------------------------------------
def _labels_of(rs, rows, NC):
    return (rs.uniform(size=(rows, NC)) < 0.3).astype(np.float32)


def _random_table(rs, L3s, NC):
    cols = []
    for L3 in L3s:
        for _ in range(NC):
            edges = np.sort(rs.choice(np.arange(0, L3 + 1), size=min(2 * rs.randint(0, 4), L3 + 1), replace=False))
            cols.append([(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])])
    return rn.table(cols, pad=2)


def test_windowed_relabel_is_in_place_and_transform_returns_the_statements_slices():
    from dcase2019_task4_amd.longrec import WindowedFeatureSet
    T, P8, NC = 64, 8, 10
    rs = np.random.RandomState(8)
    lengths = [64, 50, 152, 40, 400]                                           # two clips | a recording, one shorter than a window, a long one
    feats = [(np.abs(rs.standard_normal((n, 64))) * 3.0).astype(np.float32) for n in lengths]
    rows = [max(1, n // P8) for n in lengths]
    labels = [_labels_of(rs, r, NC) for r in rows]
    ws = WindowedFeatureSet.from_arrays(feats, labels, (2, 3), (1, 1), T, [False, True], pooling_time_ratio=P8, augment_type=None)
    items = [2, 3, 0]
    L3s = [rows[i] for i in items]
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    ptr, pairs = _random_table(rs, L3s, NC)
    assert ptr[-1] > 20
    want, werr, _ = rn.rasterize(ptr, pairs, f0, 3, NC, np.full((int(f0[-1]), NC), np.nan, np.float32))
    address, before = ws.label_pool.data_ptr(), ws.label_pool.cpu().numpy().copy()
    err = ws.relabel(items, (torch.from_numpy(ptr).cuda(), torch.from_numpy(pairs).cuda()), f0)
    assert int(err.item()) == 0 and werr == 0 and ws.label_pool.data_ptr() == address
    after = ws.label_pool.cpu().numpy()
    timeline = dict(enumerate(labels))
    for r, i in enumerate(items):
        timeline[i] = want[f0[r]:f0[r + 1]]
    for i in range(5):
        lo = int(ws.label_offset_host[i])
        rn.same_bits(after[lo:lo + rows[i]], timeline[i])                       # items 1 and 4 keep their labels bit for bit
    assert not np.array_equal(after, before)
    windows = [(2, 0), (2, 3), (2, 11), (2, 15), (2, 18), (3, 0), (3, 2), (0, 0), (1, 0), (4, 42), (4, 45)]
    clean, tgt = ws.transform(windows)
    tgt = tgt.cpu().numpy()
    for b, (i, s) in enumerate(windows):
        cut = timeline[i][s:s + T // P8]
        rn.same_bits(tgt[b], np.concatenate([cut, np.zeros((T // P8 - len(cut), NC), np.float32)]))
    # soft values and the maximum on top of what is there
    vals = torch.full((len(pairs),), 0.5, device="cuda")
    err = ws.relabel(items[:1], (torch.from_numpy(ptr[:NC + 1]).cuda(), torch.from_numpy(pairs).cuda()), f0[:2], values=vals,
                     combine="max")
    assert int(err.item()) == 0
    lo = int(ws.label_offset_host[2])
    rn.same_bits(ws.label_pool.cpu().numpy()[lo:lo + rows[2]], timeline[2])    # max(0.5, 1) = 1 where covered, the rest stays
    with pytest.raises(ValueError, match="label_rows"):
        ws.relabel([4, 3, 0], (torch.from_numpy(ptr).cuda(), torch.from_numpy(pairs).cuda()), f0)


def test_resident_relabel_is_in_place_and_gather_returns_the_new_targets():
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    T, T3, NC = 64, 8, 10
    rs = np.random.RandomState(9)
    feats = [(np.abs(rs.standard_normal((n, 64))) * 3.0).astype(np.float32) for n in (64, 70, 64, 90)]
    targets = [_labels_of(rs, T3, NC) for _ in feats]
    rset = ResidentFeatureSet.from_arrays(feats, targets, frames=T, augment_type=None)
    items, f0 = [3, 1], np.array([0, T3, 2 * T3], np.int64)
    ptr, pairs = _random_table(rs, [T3, T3], NC)
    want, werr, _ = rn.rasterize(ptr, pairs, f0, 2, NC, np.full((2 * T3, NC), np.nan, np.float32))
    address = rset.targets.data_ptr()
    err = rset.relabel(items, {"ev_ptr": torch.from_numpy(ptr).cuda(), "ev_pairs": torch.from_numpy(pairs).cuda()}, f0)
    assert int(err.item()) == 0 and rset.targets.data_ptr() == address and ptr[-1] > 10
    clean, tgt = rset.transform([0, 1, 2, 3])
    tgt = tgt.cpu().numpy()
    rn.same_bits(tgt[0], targets[0])
    rn.same_bits(tgt[2], targets[2])
    rn.same_bits(tgt[3], want[:T3])
    rn.same_bits(tgt[1], want[T3:])


# ---- 12 - 13. get_long_predictions and pseudo_label -----------------------------------------------------------------------------------
NUM, DEN = 8.0, 44100 / 511


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
    return model, lset, labels, names, feats, tl, thr


def test_get_long_predictions_defaults_reach_no_new_entry_and_return_table_reproduces_the_frame(monkeypatch):
    from dcase2019_task4_amd import inference
    model, lset, labels, names, feats, tl, thr = _long_case()
    kw = dict(batch_size=8, threshold=thr, median_window=3)
    df, table = inference.get_long_predictions(model, lset, labels, return_table=True, **kw)
    assert sorted(table) == ["ev_pairs", "ev_ptr", "timeline"] and table["timeline"] is None
    ptr, pairs = table["ev_ptr"].cpu().numpy(), table["ev_pairs"].cpu().numpy()
    assert len(df) == ptr[-1] > 30
    rows = [(labels[col % 10], on * NUM / DEN, off * NUM / DEN, names[col // 10])
            for col in range(30) for on, off in pairs[ptr[col]:ptr[col + 1]].tolist()]
    assert rows == list(df.itertuples(index=False, name=None))
    scored, table = inference.get_long_predictions(model, lset, labels, return_table=True,
                                                        min_event_score=np.quantile(tl, 0.9, axis=0).astype(np.float32), **kw)
    assert sorted(table) == ["ev_pairs", "ev_ptr", "score_max", "score_mean", "timeline"]
    n = int(table["ev_ptr"][-1].item())
    assert 0 < n == len(scored) < len(df) and table["timeline"].cpu().numpy().tobytes() == tl.tobytes()
    assert scored.score_max.to_numpy().tobytes() == table["score_max"][:n].cpu().numpy().tobytes()

    def never(*a, **k):
        raise AssertionError("a new entry point was reached with the defaults")
    monkeypatch.setattr(inference, "events_rasterize", never)
    monkeypatch.setattr(inference._lib.lib(), "sed_events_rasterize", never, raising=False)
    again = inference.get_long_predictions(model, lset, labels, **kw)
    assert again.equals(df) and (again.index == df.index).all() and list(again.columns) == list(df.columns)
    with pytest.raises(ValueError, match="return_table"):
        inference.get_long_predictions(model, lset, labels, return_table=1, **kw)


def _target_set(lset, feats, seed):
    """A windowed training set over the recordings of ``lset`` (plus two clips in front), random labels to start from."""
    from dcase2019_task4_amd.longrec import WindowedFeatureSet
    rs = np.random.RandomState(seed)
    clips = [(np.abs(rs.standard_normal((64, 64))) * 3.0).astype(np.float32) for _ in range(2)]
    L3s = np.diff(lset.rec_frame0_host).tolist()
    labels = [_labels_of(rs, 8, 10) for _ in clips] + [_labels_of(rs, L3, 10) for L3 in L3s]
    ws = WindowedFeatureSet.from_arrays(clips + list(feats), labels, (2, 3), (1, 1), 64, [False, True], augment_type=None)
    assert ws.label_rows_host.tolist() == [8, 8] + L3s
    return ws, labels


@pytest.mark.parametrize("case", ["plain", "cleaned_soft"])
def test_pseudo_label_writes_the_statements_rows_of_the_final_table(case):
    from dcase2019_task4_amd import inference
    model, lset, labels, names, feats, tl, thr = _long_case()
    kw = dict(batch_size=8, threshold=thr, median_window=3)
    soft = None
    if case == "cleaned_soft":
        kw.update(threshold_high=np.quantile(tl, 0.8, axis=0).astype(np.float32), min_event_length=0.2)
        soft = "max"
    df, table = inference.get_long_predictions(model, lset, labels, return_table=True, event_scores=soft is not None, **kw)
    ws, start = _target_set(lset, feats, 3)
    items = [4, 2, 3]                                                          # recording r -> item items[r]: equal lengths needed
    with pytest.raises(ValueError, match="label frames"):
        inference.pseudo_label(model, lset, ws, items, labels, soft=soft, **kw)
    items, address = [2, 3, 4], ws.label_pool.data_ptr()
    out = inference.pseudo_label(model, lset, ws, items, labels, soft=soft, **kw)
    ptr, pairs = table["ev_ptr"].cpu().numpy(), table["ev_pairs"].cpu().numpy()
    assert out["table"]["ev_ptr"].cpu().numpy().tobytes() == ptr.tobytes() and ptr[-1] == len(df) > 0
    np.testing.assert_array_equal(out["events_per_class"], np.diff(ptr).reshape(3, 10))
    value = None if soft is None else table["score_max"].cpu().numpy()
    f0 = lset.rec_frame0_host
    want, werr, _ = rn.rasterize(ptr, pairs, f0, 3, 10, np.full((int(f0[-1]), 10), np.nan, np.float32), value=value)
    pool = ws.label_pool.cpu().numpy()
    assert werr == 0 and ws.label_pool.data_ptr() == address
    rn.same_bits(pool[16:], want)
    rn.same_bits(pool[:16], np.concatenate(start[:2]))
    if soft is not None:
        assert set(np.unique(want)) - {0.0, 1.0} and want.max() <= 1.0
    with pytest.raises(TypeError, match="save_predictions"):
        inference.pseudo_label(model, lset, ws, items, labels, save_predictions="x.tsv")


def test_pseudo_label_with_known_tags_drops_the_classes_a_recording_does_not_hold():
    from dcase2019_task4_amd import inference
    model, lset, labels, names, feats, tl, thr = _long_case()
    kw = dict(batch_size=8, threshold=thr, median_window=3)
    ws, start = _target_set(lset, feats, 4)
    free = inference.pseudo_label(model, lset, ws, [2, 3, 4], labels, **kw)
    free_pool = ws.label_pool.cpu().numpy().copy()
    known = np.ones((3, 10), np.float32)
    known[2] = 0                                                               # the long recording holds nothing
    known[0, ::2] = 0
    out = inference.pseudo_label(model, lset, ws, [2, 3, 4], labels, known_tags=torch.from_numpy(known), **kw)
    np.testing.assert_array_equal(out["events_per_class"], free["events_per_class"] * known.astype(np.int64))
    assert free["events_per_class"][2].sum() > 0 and out["events_per_class"].sum() > 0
    pool = ws.label_pool.cpu().numpy()
    f0 = 16 + lset.rec_frame0_host
    assert (pool[f0[2]:f0[3]].view(np.uint32) == 0).all()                      # all +0.0f
    rn.same_bits(pool[f0[1]:f0[2]], free_pool[f0[1]:f0[2]])
    rn.same_bits(pool[f0[0]:f0[1]], free_pool[f0[0]:f0[1]] * known[0])
    with pytest.raises(ValueError, match="known_tags"):
        inference.pseudo_label(model, lset, ws, [2, 3, 4], labels, known_tags=np.ones((2, 10)), **kw)


# ---- 14. training on a set relabelled in place ----------------------------------------------------------------------------------------
def test_one_epoch_on_a_set_relabelled_in_place_equals_the_epoch_on_a_set_built_from_those_labels():
    from dcase2019_task4_amd.longrec import WindowedFeatureSet
    from dcase2019_task4_amd.train import train
    from tests.test_gpu_window_train import BSZ, P8, SIZES, T, _train_items
    feats, labels, sc = _train_items(False)
    n0 = SIZES[0] + SIZES[1]
    items = list(range(n0, n0 + SIZES[2]))
    L3s = [labels[i].shape[0] for i in items]
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    rs = np.random.RandomState(14)
    ptr, pairs = _random_table(rs, L3s, 10)
    want, werr, _ = rn.rasterize(ptr, pairs, f0, len(items), 10, np.full((int(f0[-1]), 10), np.nan, np.float32))
    assert werr == 0 and ptr[-1] > 20
    new = list(labels[:n0]) + [want[f0[r]:f0[r + 1]] for r in range(len(items))]

    def epoch(lab, relabel):
        ws = WindowedFeatureSet.from_arrays(feats, lab, SIZES, BSZ, T, [False, False, True], pooling_time_ratio=P8, scaler=sc, seed=5)
        if relabel:
            err = ws.relabel(items, (torch.from_numpy(ptr).cuda(), torch.from_numpy(pairs).cuda()), f0)
            assert int(err.item()) == 0
        student, _ = gu.make_model(0, dropout=0.5)
        teacher, _ = gu.make_model(1, dropout=0.5)
        opt = torch.optim.Adam(student.parameters(), lr=1e-3, betas=(0.9, 0.999))
        np.random.seed(5)
        m = train(ws, student, opt, 0, ema_model=teacher, weak_mask=ws.weak_mask, strong_mask=ws.strong_mask, log=lambda s: None)
        torch.cuda.synchronize()
        params = [p.detach().cpu().numpy().copy() for mod in (student, teacher) for p in mod.parameters()]
        student._mt_step.close()
        return params, m

    built, m_built = epoch(new, False)
    inplace, m_inplace = epoch(labels, True)
    assert all(np.isfinite(v) for v in m_built.values())
    for a, b in zip(built, inplace):
        assert a.tobytes() == b.tobytes()
    stale, _ = epoch(labels, False)                                            # the old labels train something else
    assert any(a.tobytes() != b.tobytes() for a, b in zip(built, stale))

"""-m gpu tests of sed_window_activity / sed_window_event_starts against the plain-loop statement (tests/crop_np.py) and of
``WindowedFeatureSet(sampling="events")`` built on them: window lengths, class counts, items around the window and the scan
tile, label values that are and are not active, item boundaries inside a wave, more tiles than the one-workgroup scan takes
at once, permuted slots and extreme draws, two calls and a graph replay, a relabel in place, the error bits, and one epoch
of training.

Every output lies between guard words and starts as sentinel words; everything is integer and compared exactly."""
import numpy as np
import pytest
import torch

from tests import crop_np as cn
from tests import gpu_util as gu

pytestmark = pytest.mark.gpu

TILE = 256                                                                       # label rows per workgroup of the scan passes
GUARD, SENT = 8, -0x21524111
U_MAX = 2 ** 64 - 1


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


class _Out:
    """``n`` elements of ``dtype`` between two guards, all sentinel words until something writes them."""

    def __init__(self, n, dtype):
        self.n, self.buf = n, torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + n]

    def fill(self):
        self.buf.fill_(SENT)

    def get(self):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == SENT).all() and (h[GUARD + self.n:] == SENT).all()
        return h[GUARD:GUARD + self.n].copy()


class CropCall:
    """The two entries on items given as label timelines ``labels[i]`` [R_i, NC] and their ``his``."""

    def __init__(self, labels, his, T3, NC, pool=1, clip_frames=None):
        from dcase2019_task4_amd import _lib
        self._lib, self.l = _lib, _lib.lib()
        self.labels, self.his, self.T3, self.NC, self.pool_ratio = labels, [int(h) for h in his], T3, NC, pool
        rows = np.array([len(y) for y in labels], np.int64)
        self.n, self.total = len(labels), int(rows.sum())
        self.h_row0 = np.r_[0, np.cumsum(rows)].astype(np.int64)
        self.pool = _dev(np.concatenate(labels, axis=0).reshape(self.total, NC), np.float32)
        self.row0, self.hi = _dev(self.h_row0, np.int64), _dev(self.his, np.int32)
        self.clip_frames = _dev([(h + 1) * pool for h in self.his] if clip_frames is None else clip_frames, np.int32)
        cells = (self.total + self.n) * NC
        self.A, self.B = _Out(cells, torch.int32), _Out(cells, torch.int64)
        self.W, self.present = _Out(self.n * NC, torch.int64), _Out(self.n, torch.int32)
        self.ws_bytes = self.l.sed_window_activity_ws_bytes(self.total, self.n, NC)
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")
        self.err = _Out(1, torch.int32)
        self.slots = None

    def fill(self, err0=0):
        for o in (self.A, self.B, self.W, self.present, self.err) + ((self.start, self.cls) if self.slots is not None else ()):
            o.fill()
        self.ws.fill_(0xFF)
        self.err.view.fill_(err0)

    def launch_activity(self, **kw):
        p = self._lib.ptr
        a = dict(pool=self.pool, row0=self.row0, total=self.total, n=self.n, NC=self.NC, hi=self.hi, T3=self.T3, A=self.A.view,
                 B=self.B.view, W=self.W.view, present=self.present.view, ws=self.ws, ws_bytes=self.ws_bytes, err=self.err.view)
        a.update(kw)
        return self.l.sed_window_activity(p(a["pool"]), p(a["row0"]), a["total"], a["n"], a["NC"], p(a["hi"]), a["T3"], p(a["A"]),
                                          p(a["B"]), p(a["W"]), p(a["present"]), p(a["ws"]), a["ws_bytes"], p(a["err"]),
                                          self._lib.stream_ptr())

    def set_slots(self, slot_item, u, v, m):
        self.slots = (np.asarray(slot_item, np.int64), np.asarray(u, np.uint64), np.asarray(v, np.int64), np.asarray(m, bool))
        self.slot_item, self.u = _dev(self.slots[0], np.int32), _dev(self.slots[1].view(np.int64), np.int64)
        self.v, self.m = _dev(self.slots[2], np.int32), _dev(self.slots[3], np.uint8)
        self.start, self.cls = _Out(len(self.slots[0]), torch.int32), _Out(len(self.slots[0]), torch.int32)

    def launch_starts(self, **kw):
        p = self._lib.ptr
        a = dict(u=self.u, v=self.v, m=self.m, slot_item=self.slot_item, n_slots=len(self.slots[0]), hi=self.hi,
                 clip_frames=self.clip_frames, pool_ratio=self.pool_ratio, row0=self.row0, total=self.total, n=self.n, NC=self.NC,
                 T3=self.T3, A=self.A.view, B=self.B.view, W=self.W.view, present=self.present.view, start=self.start.view,
                 cls=self.cls.view, err=self.err.view)
        a.update(kw)
        return self.l.sed_window_event_starts(p(a["u"]), p(a["v"]), p(a["m"]), p(a["slot_item"]), a["n_slots"], p(a["hi"]),
                                              p(a["clip_frames"]), a["pool_ratio"], p(a["row0"]), a["total"], a["n"], a["NC"],
                                              a["T3"], p(a["A"]), p(a["B"]), p(a["W"]), p(a["present"]), p(a["start"]),
                                              p(a["cls"]), p(a["err"]), self._lib.stream_ptr())

    def get(self):
        torch.cuda.synchronize()
        out = {k: getattr(self, k).get() for k in ("A", "B", "W", "present")}
        if self.slots is not None:
            out["start"], out["cls"] = self.start.get(), self.cls.get()
        out["err"] = int(self.err.get()[0])
        return out

    def run(self):
        self.fill()
        assert self.launch_activity() == 0, self.l.sed_last_error()
        if self.slots is not None:
            assert self.launch_starts() == 0, self.l.sed_last_error()
        return self.get()

    def want(self):
        """The statement: A / B in the entries' layout, W, the mask, and the slots' starts and classes."""
        NC = self.NC
        A = np.zeros((self.total + self.n, NC), np.int64)
        B = np.zeros((self.total + self.n, NC), np.int64)
        for i, y in enumerate(self.labels):
            a, b = cn.prefix_tables(y, NC)
            lo = int(self.h_row0[i]) + i
            A[lo:lo + len(y) + 1], B[lo:lo + len(y) + 1] = a, b
        out = {"A": A.reshape(-1), "B": B.reshape(-1)}
        slots = self.slots if self.slots is not None else (np.zeros(0, np.int64),) * 4
        start, cls, W, mask = cn.starts(self.labels, NC, self.T3, self.his, [True] * self.n, *slots)
        out.update(W=W.reshape(-1), present=mask.astype(np.int64), start=start, cls=cls)
        return out

    def check(self):
        got, want = self.run(), self.want()
        assert got["err"] == 0
        for k in ("A", "B", "W", "present") + (("start", "cls") if self.slots is not None else ()):
            g = got[k].astype(np.int64) & 0xFFFFFFFF if k == "present" else got[k].astype(np.int64)
            np.testing.assert_array_equal(g, want[k], err_msg=k)
        return got


def _bytes(out):
    return b"".join(out[k].tobytes() for k in sorted(out) if k != "err")


def _sparse(rs, R, NC, density=0.06):
    return (rs.uniform(size=(R, NC)) < density).astype(np.float32)


def _grid_items(T3, NC, seed):
    """(labels, his): items around the window length, with events at the edges, odd values, and around the scan tile.  The
    first items are short, so the first wave holds several item boundaries."""
    rs = np.random.RandomState(seed)
    zeros = lambda R: np.zeros((R, NC), np.float32)
    items = []
    y = zeros(1); y[0, 0] = 1
    items.append((y, 0))                                                         # R = 1
    y = zeros(max(1, T3 - 1)); y[-1, NC - 1] = 1
    items.append((y, 0))                                                         # R < T3: hi = 0
    items.append((zeros(50), max(0, 50 - T3)))                                   # no events
    y = zeros(50); y[0, :] = 1
    items.append((y, 70))                                                        # R shorter than L3, an event on the first row
    y = zeros(90); y[89, 0] = 1; y[40:43, NC // 2] = 1
    items.append((y, 30))                                                        # R longer than L3; the last row is out of reach
    y = zeros(90); y[89, 0] = 1
    items.append((y, max(0, 90 - T3)))                                           # an event on the last row
    y = zeros(60); y[:, NC - 1] = 1
    items.append((y, max(0, 60 - T3)))                                           # an event over the whole item
    y = zeros(100); y[10, 0] = 0.3; y[20, 0] = np.nan; y[30, 0] = -1.0; y[40, 0] = -0.0; y[99, 0] = 1e-30
    y[50:60, NC - 1] = np.nan
    items.append((y, max(0, 100 - T3)))                                          # soft, NaN, negative, -0.0
    for R in (TILE, TILE - 1, TILE + 1, 3 * TILE + 17):
        items.append((_sparse(rs, R, NC), max(0, R - T3)))
    return [i[0] for i in items], [i[1] for i in items]


def _slots(rs, n_items, per_item=6):
    """Permuted slots with random and extreme draws, event-aware and uniform."""
    slot_item = rs.permutation(np.repeat(np.arange(n_items), per_item))
    n = len(slot_item)
    u = rs.randint(0, 2 ** 32, size=n).astype(np.uint64) << np.uint64(32) | rs.randint(0, 2 ** 32, size=n).astype(np.uint64)
    u[::5], u[1::5] = 0, U_MAX
    v = rs.randint(0, 2 ** 31, size=n)
    v[::7] = 2 ** 31 - 1
    m = rs.uniform(size=n) < 0.7
    return slot_item, u, v, m


@pytest.mark.parametrize("T3", [4, 78])
@pytest.mark.parametrize("NC", [1, 10, 16])
def test_tables_starts_and_classes_against_the_statement(T3, NC):
    labels, his = _grid_items(T3, NC, 10 * T3 + NC)
    call = CropCall(labels, his, T3, NC)
    call.set_slots(*_slots(np.random.RandomState(T3 + NC), len(labels)))
    got = call.check()
    assert (got["cls"] >= 0).sum() > 10 and (got["cls"] == -1).sum() > 10
    assert int(got["present"][2]) == 0                                           # no events
    assert (got["W"].reshape(-1, NC)[4, 0] == 0) == (T3 == 4)                    # hi = 30: no window of 4 reaches row 89 or 40


def test_more_tiles_than_one_scan_step_twice_and_one_graph_replay():
    """1 030 tiles: the one-workgroup scan takes 1 024 at a step, the last item crosses that edge; an item of 70 000 mostly
    active rows takes B beyond 2^31."""
    NC, T3 = 1, 4
    rs = np.random.RandomState(6)
    rows = [70000]
    while sum(rows) < 255000:
        rows.append(int(rs.randint(1, 3000)))
    rows.append(1030 * TILE - 100 - sum(rows))
    labels = [_sparse(rs, R, NC, 0.9 if k == 0 else 0.05) for k, R in enumerate(rows)]
    his = [max(0, R - T3) for R in rows]
    call = CropCall(labels, his, T3, NC)
    assert call.total > 1024 * TILE and call.h_row0[-2] < 1024 * TILE
    call.set_slots(*_slots(rs, len(rows), 4))
    eager = call.check()
    assert eager["B"].max() > 2 ** 31
    again = call.run()
    assert again["err"] == 0 and _bytes(again) == _bytes(eager)
    graph = torch.cuda.CUDAGraph()
    call.fill()
    with torch.cuda.graph(graph):
        assert call.launch_activity() == 0 and call.launch_starts() == 0
    call.fill()
    graph.replay()
    replay = call.get()
    assert replay["err"] == 0 and _bytes(replay) == _bytes(eager)


# ---- the error bits ---------------------------------------------------------------------------------------------------------------------
def _err_call(NC=3):
    rs = np.random.RandomState(2)
    rows = [40, 300, 7]
    call = CropCall([_sparse(rs, R, NC, 0.2) for R in rows], [36, 296, 3], 4, NC, pool=8)
    call.set_slots([0, 1, 2, 1, 0, 2], [0, U_MAX, 5 << 60, 1 << 63, 9 << 59, 3 << 61], [0, 1, 2, 3, 4, 5], [1, 1, 1, 0, 1, 1])
    return call


def _untouched(x):
    return (np.asarray(x) == SENT).all()


def test_bad_host_arguments_return_before_any_launch():
    call = _err_call()
    call.fill(err0=0)
    bad = [dict(pool=None), dict(row0=None), dict(hi=None), dict(A=None), dict(B=None), dict(W=None), dict(present=None),
           dict(ws=None), dict(err=None), dict(total=0), dict(total=2 ** 31), dict(n=0), dict(NC=0), dict(T3=0),
           dict(ws_bytes=call.ws_bytes + 8), dict(ws_bytes=call.ws_bytes - 8)]
    for kw in bad:
        assert call.launch_activity(**kw) != 0, kw
    bad = [dict(u=None), dict(v=None), dict(m=None), dict(slot_item=None), dict(start=None), dict(cls=None), dict(err=None),
           dict(clip_frames=None), dict(n_slots=-1), dict(pool_ratio=0), dict(T3=0), dict(NC=0), dict(n=0), dict(total=0)]
    for kw in bad:
        assert call.launch_starts(**kw) != 0, kw
    got = call.get()
    assert got["err"] == 0 and all(_untouched(got[k]) for k in ("A", "B", "W", "present", "start", "cls"))
    assert call.l.sed_window_activity_ws_bytes(0, 1, 1) == 0 and call.l.sed_window_activity_ws_bytes(10, 0, 1) == 0
    assert call.l.sed_window_activity_ws_bytes(10, 1, 0) == 0


def test_more_than_16_classes_raise_bit_8_and_write_nothing():
    NC = 17
    call = CropCall([np.ones((20, NC), np.float32)], [16], 4, NC)
    call.set_slots([0, 0], [0, U_MAX], [0, 1], [1, 1])
    got = call.run()
    assert got["err"] == 8 and all(_untouched(got[k]) for k in ("A", "B", "W", "present", "start", "cls"))
    call.fill()
    assert call.launch_starts() == 0                                             # each entry raises it on its own
    got = call.get()
    assert got["err"] == 8 and _untouched(got["start"]) and _untouched(got["cls"])


@pytest.mark.parametrize("bad_item", [-1, 3, 2 ** 31 - 1])
def test_a_slot_item_outside_the_set_raises_bit_16_and_leaves_the_other_slots_right(bad_item):
    call = _err_call()
    want = call.check()
    slot_item = call.slots[0].copy()
    slot_item[2] = bad_item
    call.slot_item = _dev(slot_item, np.int32)
    got = call.run()
    assert got["err"] == 16 and got["start"][2] == SENT and got["cls"][2] == SENT
    keep = np.arange(6) != 2
    np.testing.assert_array_equal(got["start"][keep], want["start"][keep])
    np.testing.assert_array_equal(got["cls"][keep], want["cls"][keep])


@pytest.mark.parametrize("entry,value", [(1, 400), (2, 30), (3, 10 ** 6), (0, -1)])
def test_broken_label_rows_raise_bit_16_and_write_nothing_for_the_item(entry, value):
    call = _err_call()
    want = call.check()
    row0 = call.h_row0.copy()
    row0[entry] = value
    call.row0 = _dev(row0, np.int64)
    got = call.run()
    assert got["err"] == 16
    ok = np.array([0 <= row0[i] < row0[i + 1] <= call.total for i in range(3)])
    assert not ok.all()
    W, present = got["W"].reshape(3, -1), got["present"]
    for i in range(3):
        if not ok[i]:
            assert _untouched(W[i]) and present[i] == SENT
            assert _untouched(got["start"][call.slots[0] == i]) and _untouched(got["cls"][call.slots[0] == i])
        else:
            assert (got["start"][call.slots[0] == i] >= 0).all() and (got["start"][call.slots[0] == i] <= call.his[i]).all()
    if entry == 3:                                                               # items 0 and 1 keep their rows: their results stand
        for k in ("start", "cls"):
            np.testing.assert_array_equal(got[k][call.slots[0] != 2], want[k][call.slots[0] != 2])


def test_a_start_hi_outside_its_item_raises_bit_32():
    call = _err_call()
    want = call.check()
    call.hi = _dev([36, -1, 3], np.int32)                                        # negative: both entries refuse the item
    got = call.run()
    assert got["err"] == 32 and _untouched(got["W"].reshape(3, -1)[1]) and got["present"][1] == SENT
    assert _untouched(got["start"][call.slots[0] == 1])
    np.testing.assert_array_equal(got["start"][call.slots[0] != 1], want["start"][call.slots[0] != 1])
    call.hi = _dev(call.his, np.int32)
    frames = [(h + 1) * 8 for h in call.his]
    frames[2] = call.his[2] * 8                                                  # hi * pool == the item's frames: one too far
    call.clip_frames = _dev(frames, np.int32)
    got = call.run()
    assert got["err"] == 32 and _untouched(got["start"][call.slots[0] == 2]) and _untouched(got["cls"][call.slots[0] == 2])
    np.testing.assert_array_equal(got["start"][call.slots[0] != 2], want["start"][call.slots[0] != 2])
    np.testing.assert_array_equal(got["W"], want["W"])                           # the activity does not look at the frames
    frames[2] += 1
    call.clip_frames = _dev(frames, np.int32)
    got = call.run()
    assert got["err"] == 0 and _bytes(got) == _bytes(want)


# ---- the set ----------------------------------------------------------------------------------------------------------------------------
def _set(event_fraction=0.5, seed=7):
    from dcase2019_task4_amd.longrec import WindowedFeatureSet
    T, P8, NC = 64, 8, 10
    rs = np.random.RandomState(8)
    lengths = [64, 50, 152, 40, 400, 2600]                                       # two clips | recordings: long, shorter than a window, longer
    feats = [(np.abs(rs.standard_normal((n, 64))) * 3.0).astype(np.float32) for n in lengths]
    labels = [_sparse(rs, max(1, n // P8), NC, 0.05) for n in lengths]
    ws = WindowedFeatureSet.from_arrays(feats, labels, (2, 4), (1, 2), T, [False, True], pooling_time_ratio=P8, augment_type=None,
                                        sampling="events", seed=seed, event_fraction=event_fraction)
    return ws, labels


@pytest.mark.parametrize("fraction", [0.0, 0.5, 1.0])
def test_slot_starts_classes_and_weights_of_a_set_equal_the_statement(fraction):
    ws, labels = _set(fraction)
    for epoch in (0, 3):
        start, cls, W, mask = cn.set_starts(ws, epoch, labels)
        got = ws.slot_starts(epoch)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, start)
        np.testing.assert_array_equal(ws.slot_classes(epoch), cls)
        gW, gmask = ws.event_weights()
        np.testing.assert_array_equal(gW, W)
        np.testing.assert_array_equal(gmask, mask)
        np.random.seed(4)
        table = ws.epoch_table(epoch)                                            # the unchanged path from the starts to the table
        assert table.dtype == np.int32 and set(map(tuple, table.reshape(-1, 2))) <= set(zip(ws.slot_item, start))
    assert (start[ws.slot_item < 2] == 0).all() and (cls[ws.slot_item < 2] == -1).all()
    aware = (ws.slot_item >= 2) & (mask[ws.slot_item] != 0)                      # slots that can be drawn for a class
    assert aware.sum() > 50 and (cls[~aware] == -1).all()
    assert ((cls[aware] >= 0).any(), (cls[aware] == -1).any()) == (fraction > 0, fraction < 1)


def test_a_relabel_in_place_moves_the_next_draw():
    from tests import rasterize_np as rn
    ws, labels = _set(1.0)
    before = ws.slot_starts(0)
    np.testing.assert_array_equal(before, cn.set_starts(ws, 0, labels)[0])
    items = [5, 2]
    L3s = [len(labels[i]) for i in items]
    f0 = np.r_[0, np.cumsum(L3s)].astype(np.int64)
    cols = []
    for L3 in L3s:
        for c in range(10):
            cols.append([(L3 - 9, L3 - 2)] if c == 3 else [])                   # one event of class 3 near the end of each
    ptr, pairs = rn.table(cols, pad=2)
    address = ws.label_pool.data_ptr()
    err = ws.relabel(items, (torch.from_numpy(ptr).cuda(), torch.from_numpy(pairs).cuda()), f0)
    assert int(err.item()) == 0 and ws.label_pool.data_ptr() == address
    new = list(labels)
    for i, L3 in zip(items, L3s):
        new[i] = np.zeros((L3, 10), np.float32)
        new[i][L3 - 9:L3 - 2, 3] = 1
    start, cls, W, mask = cn.set_starts(ws, 0)                                   # the statement on the pool as it is now
    np.testing.assert_array_equal(start, cn.set_starts(ws, 0, new)[0])
    after = ws.slot_starts(0)
    np.testing.assert_array_equal(after, start)
    np.testing.assert_array_equal(ws.slot_classes(0), cls)
    moved = np.isin(ws.slot_item, items)
    assert (after[moved] != before[moved]).any() and (cls[moved] == 3).all() and (after[~moved] == before[~moved]).all()
    assert mask[5] == mask[2] == 8


def test_one_epoch_with_event_starts_equals_the_epoch_fed_the_statements_table():
    from dcase2019_task4_amd.train import train
    from tests.test_gpu_window_train import _train_set

    def epoch(statement):
        ws = _train_set(sampling="events")
        if statement:
            tables = {}
            ws.slot_starts = lambda e: tables.setdefault(e, cn.set_starts(ws, e)[0])
        student, _ = gu.make_model(0, dropout=0.5)
        teacher, _ = gu.make_model(1, dropout=0.5)
        opt = torch.optim.Adam(student.parameters(), lr=1e-3, betas=(0.9, 0.999))
        np.random.seed(5)
        m = train(ws, student, opt, 0, ema_model=teacher, weak_mask=ws.weak_mask, strong_mask=ws.strong_mask, log=lambda s: None)
        torch.cuda.synchronize()
        params = [p.detach().cpu().numpy().copy() for mod in (student, teacher) for p in mod.parameters()]
        tabs = {e: t.copy() for e, t in student._mt_frontend.host_tables.items()}
        student._mt_step.close()
        return params, m, tabs, ws

    device, m_device, t_device, ws = epoch(False)
    stated, m_stated, t_stated, _ = epoch(True)
    assert all(np.isfinite(v) for v in m_device.values())
    assert sorted(t_device) == sorted(t_stated) and all(t_device[e].tobytes() == t_stated[e].tobytes() for e in t_device)
    for a, b in zip(device, stated):
        assert a.tobytes() == b.tobytes()
    cls = ws.slot_classes(0)
    assert (cls >= 0).any() and (cls[ws.slot_item < 20] == -1).all()

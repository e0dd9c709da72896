"""CPU checks of event-aware crop sampling: the plain-loop statement (tests/crop_np.py) on hand cases and against its own
invariants, and the host side of ``WindowedFeatureSet(sampling="events")`` - the draws, the argument checks, the refusal of a
CPU set - with the tables of "random" and "grid" pinned to the statement they had before (tests/window_np.py)."""
import numpy as np
import pytest

from dcase2019_task4_amd import _lib
from dcase2019_task4_amd.longrec import SAMPLINGS, WindowedFeatureSet
from tests import crop_np as cn
from tests import window_np as wn

FRAMES, POOL, T3 = 32, 4, 8
LENGTHS = [1, 31, 32, 33, 100, 259]
U_MAX = 2 ** 64 - 1


def _timeline(R, events, nclass=2):
    y = np.zeros((R, nclass), np.float32)
    for c, on, off in events:
        y[on:off, c] = 1
    return y


def test_prefix_tables_by_hand():
    y = np.array([[0.3], [np.nan], [-1.0], [1.0], [-0.0], [2.0]], np.float32)
    A, B = cn.prefix_tables(y, 1)
    assert [r[0] for r in A] == [0, 1, 1, 1, 2, 2, 3]                    # soft counts; NaN, negative and -0.0 do not
    assert [r[0] for r in B] == [0, 0, 1, 2, 3, 5, 7]


def test_window_sums_follow_from_the_prefix_tables():
    """C_c(s) = B(s + 1 + T3) - B(T3) - B(s + 1) with A, B extended beyond R: the identity the device reads C through."""
    rs = np.random.RandomState(0)
    for R, t3, hi in [(1, 4, 0), (3, 4, 0), (9, 4, 5), (9, 4, 12), (40, 8, 32), (5, 8, 30)]:
        y = (rs.uniform(size=(R, 3)) < 0.4).astype(np.float32)
        A, B = cn.prefix_tables(y, 3)
        C, W, mask = cn.item_weights(y, 3, t3, hi)

        def Bx(x, c):
            return B[x][c] if x <= R else B[R][c] + (x - R) * A[R][c]
        for c in range(3):
            assert [Bx(s + 1 + t3, c) - Bx(t3, c) - Bx(s + 1, c) for s in range(hi + 1)] == C[c]
            assert W[c] == C[c][hi] and bool(mask >> c & 1) == (W[c] > 0)


def test_extreme_draws_give_the_first_and_the_last_start_with_activity():
    y = _timeline(60, [(0, 20, 23), (0, 40, 41), (1, 59, 60)])
    hi = 60 - T3
    C, W, mask = cn.item_weights(y, 2, T3, hi)
    assert mask == 3 and W[0] == 3 * T3 + T3 and W[1] == 1               # every active row is covered by T3 windows; the last row by one
    assert cn.slot_start(C, W, hi, True, 0, 0, True) == (20 - T3 + 1, 0)
    assert cn.slot_start(C, W, hi, True, U_MAX, 0, True) == (40, 0)
    assert cn.slot_start(C, W, hi, True, 0, 1, True) == (hi, 1) == cn.slot_start(C, W, hi, True, U_MAX, 3, True)
    # m false: the uniform rule, whatever the labels hold
    assert cn.slot_start(C, W, hi, True, 0, 0, False) == (0, -1) and cn.slot_start(C, W, hi, True, U_MAX, 0, False) == (hi, -1)
    assert cn.slot_start(C, W, hi, True, 2 ** 63, 0, False) == ((hi + 1) // 2, -1)


def test_an_item_without_events_falls_back_to_the_uniform_rule_and_a_plain_item_starts_at_zero():
    y = np.array([[0.0, -1.0, np.nan]] * 30, np.float32)
    C, W, mask = cn.item_weights(y, 3, T3, 22)
    assert mask == 0 and W == [0, 0, 0]
    for u in (0, 12345 << 40, U_MAX):
        assert cn.slot_start(C, W, 22, True, u, 7, True) == ((u * 23) >> 64, -1)
        assert cn.slot_start(C, W, 22, False, u, 7, True) == (0, -1)


def _set(sampling, seed=3, event_fraction=0.5, windowed=(False, True)):
    rs = np.random.RandomState(5)
    lengths = LENGTHS * 2
    feats = [np.abs(rs.standard_normal((n, 4))).astype(np.float32) for n in lengths]
    labels = [(rs.uniform(size=(max(1, n // POOL), 3)) < 0.15).astype(np.float32) for n in lengths]
    labels[9][:] = 0                                                     # an item without events in the windowed stream
    ws = WindowedFeatureSet.from_arrays(feats, labels, [6, 6], [2, 3], FRAMES, list(windowed), pooling_time_ratio=POOL,
                                        sampling=sampling, seed=seed, device="cpu", event_fraction=event_fraction)
    return ws, labels


@pytest.mark.parametrize("fraction", [0.0, 0.5, 1.0])
def test_every_event_mode_window_holds_an_active_frame_of_its_class(fraction):
    ws, labels = _set("events", event_fraction=fraction)
    for epoch in range(3):
        start, cls, W, mask = cn.set_starts(ws, epoch, labels)
        hi = ws.start_hi_host[ws.slot_item]
        assert (start >= 0).all() and (start <= hi).all()
        assert (start[~ws.item_windowed[ws.slot_item]] == 0).all() and (cls[~ws.item_windowed[ws.slot_item]] == -1).all()
        for j, i in enumerate(ws.slot_item):
            if cls[j] >= 0:
                assert (labels[i][start[j]:start[j] + ws.T3, cls[j]] > 0).any() and mask[i] >> cls[j] & 1
        assert (cls[ws.slot_item == 9] == -1).all()
        u, _, m = cn.draws(ws.seed, epoch, len(start), fraction)
        if fraction == 0.0:
            assert not m.any() and (cls == -1).all()
            uniform = np.array([(int(x) * (int(h) + 1)) >> 64 for x, h in zip(u, hi)])
            np.testing.assert_array_equal(start[ws.item_windowed[ws.slot_item]], uniform[ws.item_windowed[ws.slot_item]])
        if fraction == 1.0:
            holds = ws.item_windowed[ws.slot_item] & (mask[ws.slot_item] != 0)
            assert m.all() and holds.sum() > 10 and (cls[holds] >= 0).all() and (cls[~holds] == -1).all()


def test_the_draws_depend_on_seed_and_epoch_only():
    a, _ = _set("events", seed=3)
    b, _ = _set("events", seed=3, windowed=(True, True))                 # another slot layout draws a prefix-compatible stream
    for epoch in (0, 4):
        want = cn.draws(3, epoch, len(a.slot_item), 0.5)
        np.random.seed(epoch)                                            # the global generator is not consulted
        got = a.event_draws(epoch)
        np.random.seed(99)
        again = a.event_draws(epoch)
        for w, g, h in zip(want, got, again):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes() == h.tobytes()
        assert got[0].dtype == np.uint64 and got[1].max() < 2 ** 31 and got[1].min() >= 0
        assert len(b.event_draws(epoch)[0]) == len(b.slot_item)
    assert a.event_draws(0)[0].tobytes() != a.event_draws(1)[0].tobytes()
    c, _ = _set("events", seed=4)
    assert a.event_draws(0)[0].tobytes() != c.event_draws(0)[0].tobytes()


def test_events_is_a_sampling_and_refuses_a_cpu_set():
    assert SAMPLINGS == ("random", "grid", "events")
    ws, _ = _set("events")
    assert ws.event_fraction == 0.5
    for call in (lambda: ws.slot_starts(0), lambda: ws.epoch_windows(0), ws.event_weights, lambda: ws.slot_classes(0)):
        with pytest.raises(_lib.SedError, match="GPU"):
            call()
    plain, _ = _set("random")
    with pytest.raises(ValueError, match="events"):
        plain.slot_classes(0)


@pytest.mark.parametrize("bad", [-0.01, 1.5, float("nan")])
def test_event_fraction_outside_the_unit_interval_is_refused(bad):
    with pytest.raises(ValueError, match="event_fraction"):
        _set("events", event_fraction=bad)


@pytest.mark.parametrize("sampling", ["random", "grid"])
def test_random_and_grid_tables_are_what_they_were(sampling):
    """The statement these samplings had before "events" existed (tests/window_np.py), whatever event_fraction says."""
    ws, _ = _set(sampling, event_fraction=1.0)
    other, _ = _set(sampling)
    lengths, windowed = LENGTHS * 2, [False] * 6 + [True] * 6
    for epoch in range(3):
        want = np.concatenate(wn.item_starts(lengths, windowed, FRAMES, POOL, ws.hop3, sampling, 3, epoch)).astype(np.int64)
        got = ws.slot_starts(epoch)
        assert got.dtype == np.int64 and got.tobytes() == want.tobytes() == other.slot_starts(epoch).tobytes()
        np.random.seed(11)
        t = ws.epoch_table(epoch)
        np.random.seed(11)
        assert t.tobytes() == other.epoch_table(epoch).tobytes()
    assert ws._crop is None                                              # nothing of the event-aware path was built


def test_the_abi_lists_the_three_entries():
    assert {"sed_window_activity", "sed_window_event_starts", "sed_window_activity_ws_bytes"} <= set(_lib.exported_symbols())

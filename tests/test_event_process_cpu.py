"""CPU checks of minimum event length and gap merging: the plain-loop statement (tests/event_process_np.py) against its
independent frame-domain statement on decoded tables, hand cases, idempotence and the identity, the seconds -> frames rounding
of inference.process_points, and the ABI of sed_events_process."""
import os
import re

import numpy as np
import pytest

from tests import event_process_np as ep
from tests import stitch_np
from tests.hysteresis_np import smooth_timeline

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [(m, g) for m in range(-1, 8) for g in range(-1, 8)]


def _decoded_lists(n=60):
    """Event lists of decoded random timelines (tests/stitch_np.decode: every gap is at least 1 frame) with their lengths."""
    out = []
    for seed in range(n):
        rs = np.random.RandomState(seed)
        L = int(rs.randint(1, 90))
        tl = smooth_timeline(1000 + seed, L, 2) if seed % 2 else rs.uniform(size=(L, 2)).astype(np.float32)
        _, ptr, pairs = stitch_np.decode(tl, np.array([0, L], np.int64), np.full(2, rs.uniform(0.3, 0.7), np.float32),
                                         np.array([1, int(rs.choice([1, 3]))], np.int32))
        out += [([tuple(int(v) for v in e) for e in pairs[ptr[c]:ptr[c + 1]]], L) for c in range(2)]
    return out


def test_the_loops_are_the_raster_statement_on_decoded_tables():
    differ = total = 0
    for events, L in _decoded_lists():
        assert all(b[0] - a[1] >= 1 for a, b in zip(events, events[1:]))
        for m, g in PARAMS[::3]:
            got = [ep.process(events, m, g, order) for order in (0, 1)]
            for order in (0, 1):
                assert got[order] == ep.process_raster(events, m, g, order, L), (events, m, g, order)
            differ += got[0] != got[1]
            total += 1
    assert differ > total // 20                                                # the two orders are different operators


def test_hand_cases():
    ev = [(0, 1), (2, 3), (4, 5)]
    assert ep.process(ev, 3, 2, 0) == [] and ep.process(ev, 3, 2, 1) == [(0, 5)]          # the example of the header
    abut = [(0, 2), (2, 5), (6, 7), (7, 8), (10, 11)]
    assert ep.merge(abut, 0) == [(0, 5), (6, 8), (10, 11)]                     # g = 0 fuses abutting events only
    assert ep.merge(abut, -1) == abut and ep.merge(abut, 1) == [(0, 8), (10, 11)] and ep.merge(abut, 2) == [(0, 11)]
    assert ep.drop(abut, 2) == [(0, 2), (2, 5)] and ep.drop(abut, 0) == abut and ep.drop(abut, -3) == abut
    # order 0: the predecessor is the previous KEPT event - two long events fuse across the short ones between them
    run = [(0, 5), (6, 7), (8, 9), (10, 11), (12, 20)]
    assert ep.process(run, 3, 7, 0) == [(0, 20)] and ep.process(run, 3, 6, 0) == [(0, 5), (12, 20)]
    assert ep.process(run, 3, 0, 1) == [(0, 5), (12, 20)] and ep.process(run, 3, 1, 1) == [(0, 20)]
    assert ep.process([], 3, 2, 0) == [] and ep.process([(4, 5)], 1, 5, 1) == [(4, 5)]
    # differences in 64 bits
    far = [(-2 ** 31, -2 ** 31 + 1), (2 ** 31 - 2, 2 ** 31 - 1)]
    assert ep.process(far, 1, 2 ** 31 - 1, 0) == far and ep.process([(-2 ** 31, 2 ** 31 - 1)], 2 ** 31 - 1, -1, 0) == [(-2 ** 31, 2 ** 31 - 1)]


def test_idempotence_and_the_identity():
    for events, _ in _decoded_lists(30):
        assert ep.process(events, 0, -1, 0) == events and ep.process(events, -4, -1, 1) == events
        for m, g in PARAMS[::5]:
            for order in (0, 1):
                once = ep.process(events, m, g, order)
                assert ep.process(once, m, g, order) == once


def test_process_table_takes_the_parameters_of_its_point_and_class_and_the_fast_form_agrees():
    rs = np.random.RandomState(3)
    K, n_rec, NC = 3, 2, 3
    cols = []
    for _ in range(K * n_rec * NC):
        on = np.cumsum(rs.randint(1, 6, size=rs.randint(0, 12)))
        cols.append([(int(a), int(a + rs.randint(1, 4))) for a in on * 4])
    ptr = np.r_[0, np.cumsum([len(c) for c in cols])].astype(np.int64)
    pairs = np.asarray([e for c in cols for e in c], np.int32).reshape(-1, 2)
    min_len, max_gap = rs.randint(-1, 4, size=(K, NC)), rs.randint(-1, 12, size=(K, NC))
    for order in (0, 1):
        out_ptr, out_pairs = ep.process_table(ptr, pairs, n_rec, NC, min_len, max_gap, order)
        for col, events in enumerate(cols):
            k, c = col // (n_rec * NC), col % NC
            want = ep.process(events, min_len[k, c], max_gap[k, c], order)
            assert [tuple(e) for e in out_pairs[out_ptr[col]:out_ptr[col + 1]]] == want
        fast = ep.process_table_fast(ptr, pairs, n_rec, NC, min_len, max_gap, order)
        assert fast[0].tobytes() == out_ptr.tobytes() and fast[1].tobytes() == out_pairs.tobytes()
    same = ep.process_table(ptr, pairs, n_rec, NC, np.zeros((K, NC)), -np.ones((K, NC)), 0)
    assert same[0].tobytes() == ptr.tobytes() and same[1].tobytes() == pairs.tobytes()


def test_process_points_rounds_lengths_up_and_gaps_down():
    from dcase2019_task4_amd.inference import process_points
    fs = 8 * 511 / 44100                                                       # the label frame of the default configuration
    for n in (1, 2, 3, 27, 1000):
        for seconds, want_len, want_gap in ((n * fs, n, n), ((n - 0.5) * fs, n, n - 1), ((n + 0.5) * fs, n + 1, n)):
            min_len, max_gap = process_points([seconds], [seconds], 3, fs, 1)
            assert min_len.dtype == np.int32 and max_gap.dtype == np.int32 and min_len.shape == (1, 3) == max_gap.shape
            assert (min_len == want_len).all() and (max_gap == want_gap).all(), (n, seconds)
    min_len, max_gap = process_points([0.25], [0.15], 2, fs, 1)                # ceil(2.697) and floor(1.618)
    assert min_len.tolist() == [[3, 3]] and max_gap.tolist() == [[1, 1]]
    # entries: K or one, scalars or one value per class; None disables
    min_len, max_gap = process_points([0.0, [fs, 2 * fs]], [3 * fs], 2, fs, 2)
    assert min_len.tolist() == [[0, 0], [1, 2]] and max_gap.tolist() == [[3, 3], [3, 3]]
    min_len, max_gap = process_points(None, [0.0], 2, fs, 3)
    assert (min_len == 0).all() and (max_gap == 0).all() and min_len.shape == (3, 2)
    min_len, max_gap = process_points([fs], None, 2, fs, 3)
    assert (min_len == 1).all() and (max_gap == -1).all()


def test_process_points_refuses_bad_seconds_and_lengths():
    from dcase2019_task4_amd.inference import process_points
    for bad in ([-0.1], [float("nan")], [[0.1, -1.0]], [0.1, 0.2], [[0.1, 0.2, 0.3]], [float("inf")]):
        with pytest.raises(ValueError):
            process_points(bad, None, 2, 0.1, 3)
        with pytest.raises(ValueError):
            process_points(None, bad, 2, 0.1, 3)
    with pytest.raises(ValueError):
        process_points([0.1], [0.1], 2, 0.0, 1)


def test_the_two_symbols_are_bound_and_declared():
    from dcase2019_task4_amd import _lib
    header = open(os.path.join(REPO, "include", "dcase_sed.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    l = _lib.lib()
    for name in ("sed_events_process_ws_bytes", "sed_events_process"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.exported_symbols() and hasattr(l, name)
    # argument validation that needs no GPU
    assert l.sed_events_process_ws_bytes(1 << 31, 4) == 0 and l.sed_events_process_ws_bytes(8, 0) == 0
    assert b"pairs_capacity" in l.sed_last_error()
    assert l.sed_events_process_ws_bytes(0, 1) == 2 * 4 and l.sed_events_process_ws_bytes(257, 6) == 2 * 2 * 4 * 8 + 2 * 3 * 4
    from dcase2019_task4_amd.inference import events_process
    import torch
    with pytest.raises(_lib.SedError):
        events_process(torch.zeros(2, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int32), 1, 1, [[0]], [[-1]])
    with pytest.raises(ValueError):
        events_process(torch.zeros(2, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int32), 1, 1, [[0]], [[-1]], order="x")

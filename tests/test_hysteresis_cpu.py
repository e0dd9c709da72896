"""CPU-side checks of the two-threshold (hysteresis) decode's definition (include/dcase_sed.h; tests/hysteresis_np.py is its
plain-loop statement): at median window 1 it is frame-domain hysteresis (scipy's connected components of the low decisions
that hold a high decision), for every window the high events nest in the low ones - what makes the event-domain rule exact -,
equal thresholds keep everything, and the Python entry refuses thr_hi < thr_lo before any device work."""
import numpy as np
import pytest
from scipy import ndimage

from tests import hysteresis_np as hy
from tests.hysteresis_np import smooth_timeline
from tests import stitch_np


CASES = [(s, L) for s, L in enumerate([1, 2, 3, 17, 64, 257, 600, 1100])]


def _pair(tl, seed):
    rs = np.random.RandomState(100 + seed)
    lo = np.quantile(tl, rs.uniform(0.3, 0.6), axis=0).astype(np.float32)
    hi = np.maximum(np.quantile(tl, rs.uniform(0.6, 0.95), axis=0).astype(np.float32), lo)
    return lo, hi


@pytest.mark.parametrize("seed,L", CASES)
def test_window_1_is_frame_domain_hysteresis(seed, L):
    tl = smooth_timeline(seed, L)
    lo, hi = _pair(tl, seed)
    f0 = np.array([0, L], np.int64)
    ev_ptr, ev_pairs, _, _ = hy.decode(tl, f0, lo, hi, np.ones(3, np.int32))
    for c in range(3):
        lab, n = ndimage.label(tl[:, c] > lo[c])
        want = []
        for k in range(1, n + 1):
            idx = np.flatnonzero(lab == k)
            if (tl[idx, c] > hi[c]).any():
                want.append((int(idx[0]), int(idx[-1]) + 1))
        got = [tuple(int(v) for v in e) for e in ev_pairs[ev_ptr[c]:ev_ptr[c + 1]]]
        assert got == want, c


@pytest.mark.parametrize("window", [1, 3, 8, 63])
@pytest.mark.parametrize("seed,L", CASES)
def test_high_events_nest_in_low_events(seed, L, window):
    tl = smooth_timeline(seed, L)
    lo, hi = _pair(tl, seed)
    f0 = np.array([0, L], np.int64)
    win = np.full(3, window, np.int32)
    b_lo, lo_ptr, lo_pairs = stitch_np.decode(tl, f0, lo, win)
    b_hi, hi_ptr, hi_pairs = stitch_np.decode(tl, f0, hi, win)
    assert not (b_hi > b_lo).any()                                             # no frame where the high decision exceeds the low one
    for c in range(3):
        for on, off in hi_pairs[hi_ptr[c]:hi_ptr[c + 1]]:
            inside = [(a, b) for a, b in lo_pairs[lo_ptr[c]:lo_ptr[c + 1]] if a <= on and off <= b]
            assert len(inside) == 1, (c, on, off)
    # ... so "some high onset inside" selects exactly the low events that overlap a high event at all
    ev_ptr, ev_pairs = hy.select(lo_ptr, lo_pairs, hi_ptr, hi_pairs)
    for c in range(3):
        want = [(int(a), int(b)) for a, b in lo_pairs[lo_ptr[c]:lo_ptr[c + 1]] if b_hi[a:b, c].any()]
        assert [tuple(int(v) for v in e) for e in ev_pairs[ev_ptr[c]:ev_ptr[c + 1]]] == want


@pytest.mark.parametrize("window", [1, 5, 63])
def test_equal_thresholds_keep_every_event(window):
    tl = np.concatenate([smooth_timeline(40, 300), smooth_timeline(41, 7)])
    f0 = np.array([0, 300, 307], np.int64)
    thr, win = np.array([0.4, 0.5, 0.6], np.float32), np.full(3, window, np.int32)
    ev_ptr, ev_pairs, (lo_ptr, lo_pairs), _ = hy.decode(tl, f0, thr, thr, win)
    assert ev_ptr.tobytes() == lo_ptr.tobytes() and ev_pairs.tobytes() == lo_pairs.tobytes() and len(ev_pairs) > 3


def test_nan_posteriors_decide_zero_at_both_thresholds():
    tl = smooth_timeline(50, 64)
    tl[10:20] = np.nan
    _, _, (lo_ptr, lo_pairs), (hi_ptr, hi_pairs) = hy.decode(tl, np.array([0, 64], np.int64), np.full(3, 0.0, np.float32),
                                                              np.full(3, 0.01, np.float32), np.ones(3, np.int32))
    for pairs in (lo_pairs, hi_pairs):
        assert all(off <= 10 or on >= 20 for on, off in pairs)


def test_both_symbols_are_bound():
    from dcase2019_task4_amd import _lib
    assert {"sed_events_hysteresis", "sed_events_hysteresis_ws_bytes"} <= set(_lib.exported_symbols())


def test_a_high_threshold_below_the_low_one_raises_before_any_device_work():
    import torch
    from dcase2019_task4_amd import inference
    from dcase2019_task4_amd.longrec import sweep_chunks
    p = torch.zeros(2, 16, 3)                                                  # a CPU tensor: nothing can have been launched
    tables = (torch.tensor([0, 2], dtype=torch.int32), torch.tensor([0, 24], dtype=torch.int64), 24, 8)
    with pytest.raises(ValueError, match="thr_hi >= thr_lo"):
        inference.stitch_hysteresis(p, *tables, [0.5, 0.4], [0.6, 0.3], [3])
    with pytest.raises(ValueError, match="thr_hi >= thr_lo"):
        inference.stitch_hysteresis(p, *tables, [[0.5, 0.5, 0.5]], [[0.6, 0.6, 0.4]], [3])
    with pytest.raises(ValueError, match="thr_hi >= thr_lo"):
        inference.stitch_hysteresis(p, *tables, [0.5], [float("nan")], [3])
    with pytest.raises(ValueError, match="equal lengths"):
        inference.stitch_hysteresis(p, *tables, [0.5, 0.4], [0.6, 0.6, 0.6], [3])
    lo, hi, win = inference.hysteresis_points([0.2, 0.3], [0.5], [[1, 3, 5]], 3)
    assert lo.shape == hi.shape == win.shape == (2, 3) and (hi == 0.5).all() and win[1].tolist() == [1, 3, 5]
    # pairs never straddle a chunk of the sweep
    for K2, cap, limit in ((6, 10, 8 * 10 * 3), (6, 10, 8 * 10), (18, 7, 8 * 7 * 5), (2, 0, 1)):
        chunks = sweep_chunks(K2, cap, limit, pair=True)
        assert chunks[0][0] == 0 and chunks[-1][1] == K2 and all(a % 2 == 0 and b % 2 == 0 and b > a for a, b in chunks)
        assert all(chunks[i][1] == chunks[i + 1][0] for i in range(len(chunks) - 1))

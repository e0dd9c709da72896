"""What the K-operating-point sweep over long recordings states without a GPU: ``longrec.sweep_chunks`` (pure Python) and the
argument errors ``inference.stitch_sweep`` / ``metrics.validate_long`` raise before the library is touched."""
import numpy as np
import pytest
import torch

from dcase2019_task4_amd import _lib
from dcase2019_task4_amd import metrics as M
from dcase2019_task4_amd.inference import stitch_sweep, sweep_points
from dcase2019_task4_amd.longrec import MAX_SWEEP_POINTS, sweep_chunks

LIMIT = 2 ** 31 - 1024


def _check_chunks(chunks, K, cap, max_bytes, limit=LIMIT):
    assert chunks[0][0] == 0 and chunks[-1][1] == K
    assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))               # 0 .. K exactly once, in order
    for k0, k1 in chunks:
        n = k1 - k0
        assert 1 <= n <= MAX_SWEEP_POINTS
        if n > 1:                                                              # (one point is always allowed)
            assert n * cap * 8 <= max_bytes and n * cap < limit


@pytest.mark.parametrize("K,cap,max_bytes", [(50, 194_000, 1 << 30), (50, 194_000, 8 * 194_000 * 7), (50, 194_000, 8 * 194_000),
                                             (7, 1000, 8 * 1000 * 7 - 1), (1, 10, 1 << 30), (1, 10, 1), (5, 0, 0),
                                             (5000, 1, 1 << 30), (50, (LIMIT - 1) // 3, 1 << 62)])
def test_sweep_chunks_cover_every_point_once_within_both_caps(K, cap, max_bytes):
    chunks = sweep_chunks(K, cap, max_bytes)
    _check_chunks(chunks, K, cap, max_bytes)
    if cap and max_bytes >= 8 * cap:                                           # as long as possible: one more point would not fit
        n = chunks[0][1]
        assert n == K or n == MAX_SWEEP_POINTS or (n + 1) * cap * 8 > max_bytes or (n + 1) * cap >= LIMIT


def test_sweep_chunks_named_cases():
    assert sweep_chunks(50, 194_000, 1 << 30) == [(0, 50)]
    assert sweep_chunks(1, 10, 1 << 30) == [(0, 1)]
    assert sweep_chunks(7, 1000, 8 * 1000 * 3) == [(0, 3), (3, 6), (6, 7)]
    # a budget smaller than one point's table: still one point per chunk
    assert sweep_chunks(4, 1000, 100) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    # the scorers' capacity limit splits where the byte budget would not
    assert sweep_chunks(4, 1000, 1 << 40, limit=2001) == [(0, 2), (2, 4)]
    assert sweep_chunks(4, 1000, 1 << 40, limit=2000) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    with pytest.raises(ValueError):
        sweep_chunks(0, 10, 100)


def test_sweep_points_broadcasts_and_refuses():
    thr, win = sweep_points([0.1, [0.2, 0.3, 0.4]], [5], 3)
    assert thr.dtype == np.float32 and win.dtype == np.int32
    np.testing.assert_array_equal(thr, np.array([[0.1, 0.1, 0.1], [0.2, 0.3, 0.4]], np.float32))
    np.testing.assert_array_equal(win, np.full((2, 3), 5))
    with pytest.raises(ValueError):
        sweep_points([], [5], 3)


def test_stitch_sweep_argument_errors_come_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    p = torch.zeros(2, 8, 3)
    t32 = torch.tensor([0, 2], dtype=torch.int32)
    t64 = torch.tensor([0, 16], dtype=torch.int64)
    with pytest.raises(ValueError, match="equal lengths"):
        stitch_sweep(p, t32, t64, 16, 8, [0.5, 0.6], [1, 3, 5])
    with pytest.raises(ValueError, match="3 values"):
        stitch_sweep(p, t32, t64, 16, 8, [0.5, [0.1, 0.2]], [1, 3])
    with pytest.raises(ValueError, match="3 values"):
        stitch_sweep(p, t32, t64, 16, 8, [0.5, 0.6], [[1, 3, 5, 7]])
    with pytest.raises(ValueError, match="weighting"):
        stitch_sweep(p, t32, t64, 16, 8, [0.5], [1], weighting="hann")
    with pytest.raises(_lib.SedError, match="GPU"):
        stitch_sweep(p, t32, t64, 16, 8, [0.5, 0.6], [1, 3])


def test_validate_long_argument_errors_come_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    for one_blend in (True, False):
        with pytest.raises(ValueError, match="equal lengths"):
            M.validate_long(None, None, None, [0.5, 0.6], [1, 2, 3], one_blend=one_blend)
        with pytest.raises(TypeError):
            M.validate_long(None, object(), None, [0.5], one_blend=one_blend)

"""CPU checks of the recording-level weak tags of long recordings: the numpy statement (tests/weak_np.py) on hand cases, the
weak-label table, RefEvents.weak_labels, and the argument errors that must be raised before the library is touched.  The
kernels are pinned against the same statement in tests/test_gpu_long_weak.py."""
import math

import numpy as np
import pytest
import torch

from tests import long_score_np as ls
from tests import weak_np
from tests.long_util import _tables


def _inputs(n_win, T3, NC, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(size=(n_win, T3, NC)).astype(np.float32), weak_np.attention(rs, n_win, T3, NC)


def test_attention_generator_reaches_both_clamps():
    a = weak_np.attention(np.random.RandomState(0), 40, 8, 10)
    assert a.dtype == np.float32 and (a == np.float32(1e-7)).any() and (a == np.float32(1.0)).any()
    assert (a >= np.float32(1e-7)).all() and (a <= 1.0).all()


@pytest.mark.parametrize("L3", [1, 5, 8])
def test_single_window_recording_is_the_pooling_of_its_own_frames(L3):
    T3, NC = 8, 3
    p, a = _inputs(1, T3, NC, L3)
    weak, sums = weak_np.pool(p, a, [0, 1], [0, L3], 4, 1)
    for c in range(NC):
        num = math.fsum(float(p[0, v, c]) * float(a[0, v, c]) for v in range(L3))      # frames beyond L3 never enter
        den = math.fsum(float(a[0, v, c]) for v in range(L3))
        assert sums[0, c, 0] == num and sums[0, c, 1] == den
        assert weak[0, c] == np.float32(num / den)


@pytest.mark.parametrize("weighting", [0, 1])
def test_disjoint_windows_give_the_den_weighted_mean_of_the_window_tags(weighting):
    T3, NC, n = 8, 4, 3
    p, a = _inputs(n, T3, NC, 7)
    weak, sums = weak_np.pool(p, a, [0, n], [0, n * T3], T3, weighting)
    w_weak, w_sums = weak_np.pool(p, a, np.arange(n + 1), np.arange(n + 1) * T3, T3, weighting)
    mean = (w_sums[:, :, 1] * w_weak.astype(np.float64)).sum(0) / w_sums[:, :, 1].sum(0)
    np.testing.assert_allclose(weak[0], mean, rtol=4 * 2.0 ** -24, atol=0)
    np.testing.assert_allclose(sums[0, :, 1], w_sums[:, :, 1].sum(0), rtol=2.0 ** -50, atol=0)


def test_a_constant_posterior_is_its_own_tag_and_zero_mass_is_nan():
    T3, NC, hop3 = 8, 2, 3
    rec_win0, rec_frame0 = _tables([20], T3, hop3)
    a = weak_np.attention(np.random.RandomState(3), rec_win0[-1], T3, NC)
    p = np.full(a.shape, 0.25, dtype=np.float32)
    weak, _ = weak_np.pool(p, a, rec_win0, rec_frame0, hop3, 0)
    np.testing.assert_allclose(weak, 0.25, rtol=2.0 ** -22)
    weak, sums = weak_np.pool(p, np.zeros_like(a), rec_win0, rec_frame0, hop3, 0)
    assert np.isnan(weak).all() and (sums == 0).all()


def test_weak_tags_dataframe_layout_and_per_class_thresholds():
    from dcase2019_task4_amd.inference import weak_tags_dataframe
    labels = ["Dog", "Cat", "Speech"]
    weak = np.array([[0.9, 0.2, 0.6], [0.1, 0.2, 0.3], [0.5, 0.51, 0.7]], dtype=np.float32)
    df = weak_tags_dataframe(weak, ["a.wav", "b.wav", "c.wav"], labels)
    assert list(df.columns) == ["filename", "event_labels"] and df.filename.tolist() == ["a.wav", "b.wav", "c.wav"]
    assert df.event_labels.tolist() == ["Dog,Speech", "", "Cat,Speech"]                # label order; strictly above the threshold
    df = weak_tags_dataframe(torch.from_numpy(weak), ["a.wav", "b.wav", "c.wav"], labels, threshold=[0.95, 0.15, 0.65])
    assert df.event_labels.tolist() == ["Cat", "Cat", "Cat,Speech"]
    with pytest.raises(ValueError):
        weak_tags_dataframe(weak, ["a.wav"], labels)
    with pytest.raises(ValueError):
        weak_tags_dataframe(weak, ["a.wav", "b.wav", "c.wav"], labels, threshold=[0.5, 0.5])


def _ref():
    from dcase2019_task4_amd.metrics import RefEvents
    cols = [[[(0.0, 1.0), (2.0, 3.0)], [], [(0.5, 0.6)]], [[], [], []], [[], [(1.0, 9.0)], []]]
    ptr, on, off = ls.pack(cols)
    return RefEvents(ptr, on, off, ["a", "b", "c"], ["x", "y", "z"], device="cpu")


def test_ref_events_weak_labels():
    got = _ref().weak_labels()
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, [[1, 0, 1], [0, 0, 0], [0, 1, 0]])


def test_argument_errors_come_before_the_library(monkeypatch):
    from dcase2019_task4_amd import _lib, inference, metrics

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    p = torch.zeros(3, 8, 4)
    t32, t64 = torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 16], dtype=torch.int64)
    with pytest.raises(ValueError, match="weighting"):
        inference.stitch_weak(p, p, t32, t64, 16, 4, weighting="hann")
    with pytest.raises(ValueError, match="win_att"):
        inference.stitch_weak(p, torch.zeros(3, 8, 5), t32, t64, 16, 4)
    with pytest.raises(ValueError):
        inference.stitch_weak(p, p, t32, t64, 16, 9)                                  # hop3 > T3
    with pytest.raises(ValueError):
        inference.stitch_weak(torch.zeros(3, 8, 17), torch.zeros(3, 8, 17), t32, t64, 16, 4)
    with pytest.raises(ValueError):
        inference.stitch_weak(p, p, t32, t64, 2 ** 29, 4)                             # total_frames * nclass >= 2^31
    with pytest.raises(_lib.SedError, match="GPU"):
        inference.stitch_weak(p, p, t32, t64, 16, 4)                                  # CPU tensors: no fallback
    ref = _ref()
    for kw in (dict(weak_labels="from_reference"), dict(weak_labels=np.zeros((2, 3))), dict(weak_labels=np.full((3, 3), 2)),
               dict(weak_thresholds=[0.5]), dict(weak_labels="from_ref", weak_thresholds=[[0.5, 0.5]])):
        with pytest.raises(ValueError):
            metrics.validate_long(None, None, ref, **kw)


def test_f_measure_from_counts():
    from dcase2019_task4_amd.metrics import f_measure_from_counts
    got = f_measure_from_counts(np.array([[[3, 1, 1, 9], [0, 0, 0, 4], [0, 2, 0, 1]]]))
    np.testing.assert_array_equal(got, [[0.75, 0.0, 0.0]])

"""CPU checks of the long-recording path: the window plan (coverage, no empty and no superfluous window, alignment),
hop validation, the window tables of a LongRecordingSet, and a self-check of the numpy blend (tests/stitch_np.py)."""
import numpy as np
import pytest

from dcase2019_task4_amd import _lib
from dcase2019_task4_amd.inference import LongRecordingSet, check_hop_frames, default_hop_frames, window_plan
from tests import stitch_np


@pytest.mark.parametrize("frames", [16, 64, 100, 628])
def test_window_plan_covers_every_frame_with_no_empty_and_no_superfluous_window(frames):
    pool, T3 = 8, frames // 8
    for hop3 in range(1, T3 + 1):
        for L in range(1, 5 * frames + 21):
            p = window_plan(L, frames, pool, hop3)
            L3, n_w, t0, start, real = p["L3"], p["n_w"], p["t0"], p["start"], p["real"]
            assert L3 == max(1, L // pool) and n_w >= 1 and len(t0) == len(start) == len(real) == n_w
            # (plain comparisons, not np.testing: a quarter of a million plans at frames = 628)
            j = np.arange(n_w)
            assert (t0 == j * hop3).all() and (start == j * hop3 * pool).all()            # alignment: feature hop = hop3 * pool
            assert (real == np.minimum(frames, L - start)).all() and real.min() >= 1      # no window without a real frame
            # coverage: consecutive ranges touch or overlap (hop3 <= T3) and the last one reaches the end ...
            assert hop3 <= T3 and t0[-1] + T3 >= L3
            # ... and without the last window they do not: none is superfluous
            assert n_w == 1 or t0[-2] + T3 < L3


def test_window_plan_coverage_by_counting():
    """The same coverage statement, counted frame by frame on a few geometries (no reasoning about contiguity)."""
    for frames, hop3, L in [(64, 3, 300), (64, 8, 64), (64, 8, 65), (64, 8, 72), (100, 5, 517), (16, 1, 100), (64, 4, 7)]:
        p = window_plan(L, frames, 8, hop3)
        T3 = frames // 8
        n = np.zeros(p["L3"], dtype=int)
        for t in p["t0"]:
            n[t:t + T3] += 1
        assert n.min() >= 1, (frames, hop3, L)


def test_hop_frames_validation_and_default():
    assert default_hop_frames(628) == 312 and default_hop_frames(64) == 32 and default_hop_frames(16) == 8
    assert default_hop_frames(100) == 48 and default_hop_frames(8) == 8
    assert check_hop_frames(None, 628) == 312 and check_hop_frames(624, 628) == 624 and check_hop_frames(8, 628) == 8
    for bad in (0, -8, 4, 12, 632, 628, 7.5, True):
        with pytest.raises(ValueError):
            check_hop_frames(bad, 628)
    with pytest.raises(ValueError):
        default_hop_frames(7)
    f = [np.ones((20, 4), dtype=np.float32)]
    for bad in (0, 12, 72):
        with pytest.raises(ValueError):
            LongRecordingSet.from_arrays(f, 64, hop_frames=bad, device="cpu")
    assert LongRecordingSet.from_arrays(f, 64, device="cpu").hop_frames == 32


def test_window_tables_of_a_three_recording_set_by_hand():
    rs = np.random.RandomState(0)
    feats = [np.abs(rs.standard_normal((L, 4))).astype(np.float32) for L in (40, 64, 300)]
    s = LongRecordingSet.from_arrays(feats, 64, hop_frames=32, device="cpu", filenames=["a", "b", "c"])
    # T3 = 8, hop3 = 4; L3 = 5, 8, 37 -> 1, 1, 1 + ceil(29 / 4) = 9 windows
    assert (s.T3, s.hop3, s.n_rec, s.n_clips, len(s), s.max_clip_frames, s.total_frames) == (8, 4, 3, 11, 11, 64, 50)
    np.testing.assert_array_equal(s.rec_win0_host, [0, 1, 2, 11])
    np.testing.assert_array_equal(s.rec_frame0_host, [0, 5, 13, 50])
    np.testing.assert_array_equal(s.clip_offset_host, [0, 40] + [104 + 32 * j for j in range(9)])
    np.testing.assert_array_equal(s.clip_frames_host, [40, 64] + [64] * 8 + [44])
    assert s.rec_win0.dtype.is_floating_point is False and str(s.rec_win0.dtype) == "torch.int32"
    assert str(s.rec_frame0.dtype) == "torch.int64" and str(s.clip_offset.dtype) == "torch.int64"
    np.testing.assert_array_equal(s.clip_offset.numpy(), s.clip_offset_host)
    np.testing.assert_array_equal(s.clip_frames.numpy(), s.clip_frames_host)
    np.testing.assert_array_equal(s.pool.numpy(), np.concatenate([f.reshape(-1) for f in feats]))
    assert s.filenames == ["a", "b", "c"] and s.capacity(10) == 10 * (3 + 4 + 19)
    assert not s.noise and s.targets is None and s.batch_sizes is None


def test_a_cpu_set_builds_its_tables_and_refuses_to_gather():
    s = LongRecordingSet.from_arrays([np.ones((100, 4), dtype=np.float32)], 64, device="cpu")
    assert s.n_clips == 2 and len(s) == 2
    with pytest.raises(_lib.SedError):
        s.eval_batch(0, 1)


def test_numpy_uniform_blend_of_dyadic_posteriors_is_the_exact_mean():
    """Multiples of 2^-10 in [0, 1]: every partial sum of at most 8 of them is exact in float32, so the sequential float32
    sum divided by the count must equal the float64 mean rounded once."""
    rs = np.random.RandomState(3)
    T3, NC, hop3 = 8, 3, 1
    L3s = [1, 9, 30]
    n_w = [window_plan(L3 * 8, 64, 8, hop3)["n_w"] for L3 in L3s]
    rec_win0, rec_frame0 = np.r_[0, np.cumsum(n_w)], np.r_[0, np.cumsum(L3s)]
    p = (rs.randint(0, 1025, size=(sum(n_w), T3, NC)) / 1024.0).astype(np.float32)
    got = stitch_np.blend(p, rec_win0, rec_frame0, hop3, 0)
    for r, L3 in enumerate(L3s):
        for u in range(L3):
            vals = [p[rec_win0[r] + j, u - j * hop3].astype(np.float64) for j in range(n_w[r]) if 0 <= u - j * hop3 < T3]
            want = (np.sum(vals, axis=0) / len(vals)).astype(np.float32)
            np.testing.assert_array_equal(got[rec_frame0[r] + u], want)
    # a single-window recording is its window, bit for bit
    np.testing.assert_array_equal(got[:1].view(np.uint32), p[0, :1].view(np.uint32))

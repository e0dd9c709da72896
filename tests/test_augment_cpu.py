"""CPU checks of the augmentation policy (dcase2019_task4_amd/augment.py): what ``AugmentPolicy.draw`` draws, table
validation, and a training set holding a policy on a CPU device."""
import numpy as np
import pytest

from dcase2019_task4_amd import _lib
from dcase2019_task4_amd.augment import AugmentPolicy, augment_batch, identity_table, validate_table

SLICES = [slice(0, 3), slice(3, 8), slice(8, 10)]
T, T3, M = 628, 78, 64
ONE = int(np.float32(1.0).view(np.int32))


def _full(seed=7, **kw):
    args = dict(mixup_alpha=0.2, mixup_prob=0.7, shift_std=9.0, freq_mask_max=12, time_mask_max=50, seed=seed)
    args.update(kw)
    return AugmentPolicy(**args)


def _draw(pol, epoch=0, rank=0, n_steps=40):
    return pol.draw(epoch, n_steps, SLICES, T, T3, M, rank=rank)


def test_draw_is_deterministic_per_seed_rank_epoch_and_differs_across_each():
    a = _draw(_full())
    assert a.dtype == np.int32 and a.shape == (40, 10, 8) and a.flags.c_contiguous
    np.testing.assert_array_equal(a, _draw(_full()))
    for other in (_draw(_full(seed=8)), _draw(_full(), rank=1), _draw(_full(), epoch=1)):
        for col in range(8):
            if col != 3:                               # (shift_y is shift_x / 8: covered by shift_x)
                assert not np.array_equal(a[..., col], other[..., col]), col


def test_partners_stay_inside_their_stream_slice_and_non_mixing_clips_are_identity():
    a = _draw(_full())
    lam = a[..., 1].copy().view(np.float32)
    own = np.arange(10)[None, :]
    mixes = a[..., 0] != own
    assert mixes.any() and (~mixes).any()              # mixup_prob = 0.7: both kinds occur
    for s in SLICES:
        p = a[:, s, 0]
        assert p.min() >= s.start and p.max() < s.stop
        assert (p != own[:, s]).any()
    assert np.all(a[..., 1][~mixes] == ONE)
    assert np.all((lam[mixes] > 0.0) & (lam[mixes] < 1.0))
    # a slice of one clip has nobody to mix with
    one = _full().draw(0, 20, [slice(0, 1), slice(1, 4)], T, T3, M)
    assert np.all(one[:, 0, 0] == 0) and np.all(one[:, 0, 1] == ONE)


def test_shifts_move_features_and_labels_together_and_widths_respect_their_maxima():
    a = _draw(_full())
    assert T // T3 == 8
    np.testing.assert_array_equal(a[..., 2], a[..., 3] * 8)
    assert (a[..., 3] > 0).any() and (a[..., 3] < 0).any()
    assert a[..., 5].min() >= 0 and a[..., 5].max() <= 12 and a[..., 5].max() > 6
    assert a[..., 7].min() >= 0 and a[..., 7].max() <= 50 and a[..., 7].max() > 25
    assert a[..., 4].min() >= 0 and (a[..., 4] + a[..., 5]).max() <= M
    assert a[..., 6].min() >= 0 and (a[..., 6] + a[..., 7]).max() <= T
    # maxima beyond the tensor are clipped to it
    b = AugmentPolicy(freq_mask_max=1000, time_mask_max=100000).draw(0, 50, SLICES, 20, 2, 7)
    assert b[..., 5].max() <= 7 and b[..., 7].max() <= 20 and (b[..., 4] + b[..., 5]).max() <= 7
    np.testing.assert_array_equal(AugmentPolicy(shift_std=3.0).draw(0, 5, SLICES, 20, 2, 7)[..., 2],
                                  AugmentPolicy(shift_std=3.0).draw(0, 5, SLICES, 20, 2, 7)[..., 3] * 10)


def test_a_policy_with_everything_off_yields_identity_rows():
    for pol in (AugmentPolicy(), AugmentPolicy(mixup_alpha=0.2, mixup_prob=0.0), AugmentPolicy(shift_std=0)):
        assert not pol.active
        np.testing.assert_array_equal(_draw(pol), identity_table(40, 10))
    row = identity_table(10)
    np.testing.assert_array_equal(row[:, 0], np.arange(10))
    assert np.all(row[:, 1] == ONE) and not row[:, 2:].any()
    assert _full().active


def test_drawing_leaves_numpys_global_generator_untouched():
    np.random.seed(123)
    before = np.random.get_state()
    _draw(_full())
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_bad_policy_arguments_raise():
    for kw in (dict(mixup_alpha=0.0), dict(mixup_prob=1.5), dict(shift_std=-1.0), dict(freq_mask_max=-1), dict(time_mask_max=-2)):
        with pytest.raises(ValueError):
            AugmentPolicy(**kw)
    with pytest.raises(ValueError):
        _full().draw(0, 4, [slice(0, 3), slice(4, 8)], T, T3, M)           # the slices do not tile the batch


def test_bad_tables_raise():
    good = identity_table(4)
    assert validate_table(good, 4) is not None
    bad = good.copy(); bad[2, 0] = 4
    with pytest.raises(_lib.SedError):
        validate_table(bad, 4)
    bad = good.copy(); bad[0, 0] = -1
    with pytest.raises(_lib.SedError):
        validate_table(bad, 4)
    for t in (good.astype(np.int64), good[:, :7], good[:3], good.reshape(-1), good.tolist()):
        with pytest.raises(_lib.SedError):
            validate_table(t, 4)
    import torch
    with pytest.raises(_lib.SedError):                                       # no CPU path
        augment_batch(torch.zeros(4, 8, 8), None, None, good)


def test_a_cpu_set_with_a_policy_builds_its_tables_and_refuses_to_gather():
    import torch
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    rs_ = np.random.RandomState(0)
    sizes, bsz = (4, 6, 4), (2, 3, 2)
    feats = [np.abs(rs_.standard_normal((40, 8))).astype(np.float32) for _ in range(sum(sizes))]
    tgts = [rs_.uniform(size=(5, 3)).astype(np.float32) for _ in range(sum(sizes))]
    pol = _full()
    rs = ResidentFeatureSet.from_arrays(feats, tgts, sizes, bsz, frames=40, device="cpu", augment=pol)
    assert rs.augment is pol and rs.stream_slices == [slice(0, 2), slice(2, 5), slice(5, 7)]
    a = rs.augment_table(3)
    assert a.shape == (2, 7, 8) and a.dtype == np.int32
    np.testing.assert_array_equal(a, pol.draw(3, 2, rs.stream_slices, 40, 5, 8, rank=0))
    np.testing.assert_array_equal(a[..., 2], a[..., 3] * 8)
    with pytest.raises(_lib.SedError):
        rs.gather(torch.zeros(7, dtype=torch.int32), torch.empty(7, 1, 40, 8))
    plain = ResidentFeatureSet.from_arrays(feats, tgts, sizes, bsz, frames=40, device="cpu")
    assert plain.augment is None
    with pytest.raises(ValueError):
        plain.augment_table(0)
    with pytest.raises(TypeError):
        ResidentFeatureSet.from_arrays(feats, tgts, sizes, bsz, frames=40, device="cpu", augment="mixup")
    with pytest.raises(ValueError):                                          # an evaluation set never augments
        ResidentFeatureSet.from_arrays(feats, None, None, None, 40, device="cpu", augment=pol)

"""CPU-side checks of the PSDS host arithmetic (dcase2019_task4_amd.metrics.PSDS): the hand cases of the definitions, the
independent statement in tests/psds_np.py on the same hand cases and on random totals, and what needs no GPU of the counting
interface.  psds_eval is absent from this image: parity with it is unpinned; these tests pin the restated definitions."""
import numpy as np
import pandas as pd
import pytest
import torch

from tests import psds_np as ps


def _totals(tp, fp, ct=None):
    """[K, NC] TP and FP (+ [K, NC, NC] CT) -> [K, NC, 2 + NC]."""
    tp, fp = np.asarray(tp, np.int64), np.asarray(fp, np.int64)
    ct = np.zeros(tp.shape + (tp.shape[1],), np.int64) if ct is None else np.asarray(ct, np.int64)
    return np.concatenate([tp[..., None], fp[..., None], ct], axis=2)


HAND = dict(totals=_totals([[5, 2], [8, 6]], [[10, 20], [50, 40]]), n_gt=[10, 10], gt_duration=[100.0, 100.0],
            dataset_duration=3600.0)


def test_hand_case_psd_roc_and_area():
    from dcase2019_task4_amd.metrics import PSDS
    p = PSDS(["a", "b"], **HAND)
    np.testing.assert_allclose(p.tpr, [[.5, .2], [.8, .6]], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(p.fpr, [[10.0, 20.0], [50.0, 40.0]])
    np.testing.assert_array_equal(p.efpr(), p.fpr)
    assert p.ctr.shape == (2, 2, 2) and not p.ctr.any()
    axis, eff = p.psd_roc()
    np.testing.assert_array_equal(axis, [10.0, 20.0, 40.0, 50.0])
    np.testing.assert_allclose(p.class_curves(axis), [[.5, .5, .5, .8], [0, .2, .6, .6]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(eff, [.25, .35, .55, .7], rtol=0, atol=1e-12)
    assert p.psds() == pytest.approx(0.5, abs=1e-12)
    _, eff1 = p.psd_roc(alpha_st=1.0)
    np.testing.assert_allclose(eff1, [0, .2, .5, .6], rtol=0, atol=1e-12)
    assert p.psds(alpha_st=1.0) == pytest.approx(0.39, abs=1e-12)
    assert p.psds(max_efpr=45.0) == pytest.approx(12.25 / 45, abs=1e-12)
    np.testing.assert_array_equal(p.psd_roc(max_efpr=45.0)[0], [10.0, 20.0, 40.0])
    # the independent statement on the same inputs
    kw = dict(n_gt=HAND["n_gt"], gt_duration=HAND["gt_duration"], dataset_duration=3600.0)
    assert ps.psds(HAND["totals"].tolist(), **kw) == pytest.approx(0.5, abs=1e-12)
    assert ps.psds(HAND["totals"].tolist(), alpha_st=1.0, **kw) == pytest.approx(0.39, abs=1e-12)
    assert ps.psds(HAND["totals"].tolist(), max_efpr=45.0, **kw) == pytest.approx(12.25 / 45, abs=1e-12)
    # an axis without a point inside e_max: nothing is counted
    assert p.psds(max_efpr=5.0) == 0.0 and len(p.psd_roc(max_efpr=5.0)[0]) == 0


def test_alpha_ct_adds_the_mean_cross_trigger_rate_of_the_other_classes():
    from dcase2019_task4_amd.metrics import PSDS
    ct = np.zeros((1, 3, 3), np.int64)
    ct[0, 0] = [0, 4, 2]
    p = PSDS(["a", "b", "c"], _totals([[1, 1, 1]], [[10, 0, 0]], ct), [2, 2, 2], [900.0, 1800.0, 3600.0], 3600.0)
    np.testing.assert_array_equal(p.ctr[0, 0], [0.0, 8.0, 2.0])
    e = p.efpr(alpha_ct=1.0)
    assert e[0, 0] == 10 + (8 + 2) / 2 == 15.0
    assert e[0, 1] == 0.0 and e[0, 2] == 0.0
    assert p.efpr()[0, 0] == 10.0
    assert p.efpr(alpha_ct=0.5)[0, 0] == 12.5
    _, _, want = ps.psd_roc(_totals([[1, 1, 1]], [[10, 0, 0]], ct).tolist(), [2, 2, 2], [900.0, 1800.0, 3600.0], 3600.0, alpha_ct=1.0)
    assert want[0] == [15.0, 0.0, 0.0]
    # a class without reference duration contributes no cross-trigger rate; a single class has no partner at all
    q = PSDS(["a", "b"], _totals([[1, 1]], [[3, 0]], [[[0, 7], [0, 0]]]), [1, 1], [10.0, 0.0], 3600.0)
    assert q.ctr[0, 0, 1] == 0.0 and q.efpr(alpha_ct=1.0)[0, 0] == 3.0
    one = PSDS(["a"], _totals([[1]], [[7]]), [2], [10.0], 1800.0)
    assert one.efpr(alpha_ct=1.0).tolist() == [[14.0]] and one.psds() == pytest.approx(0.5 * 86 / 100, abs=1e-12)


def test_a_class_without_references_raises():
    from dcase2019_task4_amd.metrics import PSDS
    with pytest.raises(ValueError, match="b"):
        PSDS(["a", "b"], _totals([[1, 0]], [[1, 1]]), [3, 0], [1.0, 0.0], 3600.0).psds()
    with pytest.raises(ValueError):
        ps.psds(_totals([[1, 0]], [[1, 1]]).tolist(), [3, 0], [1.0, 0.0], 3600.0)
    with pytest.raises(ValueError):
        PSDS(["a", "b"], np.zeros((1, 2, 3), np.int64), [1, 1], [1.0, 1.0], 3600.0)          # totals of another width


def test_the_class_curve_is_a_monotone_staircase():
    """A point with a higher eFPR and a lower TPR does not lower the curve; points sharing an eFPR give their best TPR."""
    from dcase2019_task4_amd.metrics import PSDS
    #                      TP        FP: one class, four points
    p = PSDS(["a"], _totals([[6], [3], [8], [7]], [[10], [30], [60], [60]]), [10], [50.0], 3600.0)
    axis, eff = p.psd_roc()
    np.testing.assert_array_equal(axis, [10.0, 30.0, 60.0])
    np.testing.assert_allclose(eff, [.6, .6, .8], rtol=0, atol=1e-15)
    assert np.all(np.diff(eff) >= 0)
    assert p.psds() == pytest.approx((.6 * 20 + .6 * 30 + .8 * 40) / 100, abs=1e-12)
    np.testing.assert_array_equal(p.class_curves([0.0, 9.99, 10.0, 59.0, 1e9])[0], [0.0, 0.0, .6, .6, .8])


def test_random_totals_agree_with_the_independent_statement():
    from dcase2019_task4_amd.metrics import PSDS
    rs = np.random.RandomState(5)
    for nc, K in ((1, 3), (3, 7), (10, 50)):
        n_gt = rs.randint(1, 40, size=nc)
        tp = np.minimum(rs.randint(0, 40, size=(K, nc)), n_gt)
        fp = rs.randint(0, 60, size=(K, nc))
        ct = rs.randint(0, 9, size=(K, nc, nc)) * (1 - np.eye(nc, dtype=np.int64))
        dur = rs.uniform(10.0, 500.0, size=nc)
        dur[-1] = 0.0 if nc > 1 else dur[-1]
        p = PSDS([f"c{i}" for i in range(nc)], _totals(tp, fp, ct), n_gt, dur, 7200.0)
        for kw in (dict(), dict(alpha_ct=1.0), dict(alpha_st=1.0), dict(alpha_ct=0.5, alpha_st=0.7, max_efpr=20.0)):
            axis, eff, efpr = ps.psd_roc(_totals(tp, fp, ct).tolist(), n_gt.tolist(), dur.tolist(), 7200.0, **kw)
            np.testing.assert_allclose(p.efpr(kw.get("alpha_ct", 0.0)), efpr, rtol=1e-13, atol=0)
            got_axis, got_eff = p.psd_roc(**kw)
            # (the two round eFPR differently in the last bit, so axis values that one merges the other may keep apart)
            assert p.psds(**kw) == pytest.approx(ps.psds(_totals(tp, fp, ct).tolist(), n_gt.tolist(), dur.tolist(), 7200.0, **kw),
                                                 abs=1e-12)
            if kw.get("alpha_ct", 0.0) == 0.0:
                np.testing.assert_array_equal(got_axis, axis)
                np.testing.assert_allclose(got_eff, eff, rtol=0, atol=1e-12)


def _df(rows):
    return pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])


def test_from_counts_reads_reference_counts_and_durations_from_ref_events_on_the_cpu():
    from dcase2019_task4_amd.metrics import PSDS, PSDSCounts, RefEvents
    files, labels = ["a.wav", "b.wav", "c.wav"], ["cat", "dog"]
    df = _df([("a.wav", 0.0, 1.5, "cat"), ("b.wav", 2.0, 2.5, "cat"), ("b.wav", 1.0, 4.0, "dog"), ("c.wav", 0.25, 0.5, "dog"),
              ("c.wav", 3.0, 3.5, "dog")])
    ref = RefEvents.from_dataframe(df, files, labels, device="cpu")
    np.testing.assert_array_equal(ref.ptr_host, ref.ptr.numpy())
    np.testing.assert_array_equal(ref.onset_host, ref.onset.numpy()[:-1])
    np.testing.assert_array_equal(ref.offset_host, ref.offset.numpy()[:-1])
    totals = _totals([[1, 2], [2, 3]], [[4, 0], [9, 6]])
    p = PSDS.from_counts(totals, ref, 10.0)
    assert p.labels == labels and p.n_gt.tolist() == [2, 3] and p.gt_duration.tolist() == [2.0, 3.75]
    assert p.dataset_duration == 30.0
    np.testing.assert_array_equal(p.tpr, [[.5, 2 / 3], [1.0, 1.0]])
    np.testing.assert_array_equal(p.fpr, [[480.0, 0.0], [1080.0, 720.0]])
    assert PSDS.from_counts(totals, ref, [10.0, 4.0, 6.0]).dataset_duration == 20.0
    with pytest.raises(ValueError):
        PSDS.from_counts(totals, ref, [10.0, 4.0])
    # a PSDSCounts (here on the CPU device, where nothing can fill it) is read with host()
    counts = PSDSCounts(2, 2, "cpu")
    assert counts.totals.shape == (2, 2, 4) and counts.totals.dtype == torch.int64 and (counts.dtc, counts.gtc, counts.cttc) == (.5, .5, .3)
    counts.totals.copy_(torch.as_tensor(totals))
    np.testing.assert_array_equal(PSDS.from_counts(counts, ref, 10.0).fpr, p.fpr)
    with pytest.raises(ValueError, match="bird"):
        PSDS.from_counts(np.zeros((1, 3, 5), np.int64), RefEvents.from_dataframe(df, files, labels + ["bird"], device="cpu"), 10.0)
    with pytest.raises(ValueError):
        PSDSCounts(1, 2, "cpu", dtc=1.5)


def test_counting_on_a_cpu_device_refuses():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.metrics import RefEvents, psds_counts, psds_counts_from_events
    ref = RefEvents.from_dataframe(_df([("a.wav", 0.0, 1.0, "cat")]), ["a.wav"], ["cat"], device="cpu")
    with pytest.raises(_lib.SedError):
        psds_counts(torch.zeros(1, 8, 1), ref)
    with pytest.raises(_lib.SedError):
        psds_counts_from_events(ref, ref)


def test_library_rejects_criteria_outside_the_unit_interval():
    """Argument checks of sed_psds_counts run before anything touches a device."""
    import ctypes as C
    from dcase2019_task4_amd import _lib
    l = _lib.lib()
    one = C.c_void_p(16)                                   # never dereferenced: the call fails on its arguments
    for dtc, gtc, cttc in ((-0.1, .5, .3), (.5, 1.5, .3), (.5, .5, float("nan"))):
        assert l.sed_psds_counts(None, 1, 0, 1, 1, None, None, 0.0, 0.0, one, one, one, one, one, one, dtc, gtc, cttc, None, one,
                                 one, None) != 0
        assert b"[0, 1]" in l.sed_last_error()
    assert l.sed_psds_counts(None, 1, 0, 17, 1, None, None, 0.0, 0.0, one, one, one, one, one, one, .5, .5, .3, None, one, one,
                             None) != 0


def test_helper_criteria_on_hand_columns():
    """The ties of the definitions, in the independent statement (the device is pinned to it in tests/test_gpu_psds.py)."""
    eps = 2.0 ** -52
    d, g = (1.0, 2.0), (1.5, 3.0)
    assert ps.intersection(d, g) == 0.5 and ps.relevant_mask([d], [g], 0.5) == [True]
    assert ps.relevant_mask([d], [g], 0.5 + eps) == [False]
    assert ps.file_counts([[g]], [[d]]) == [[0, 0, 0]]                     # relevant, but 0.5 of 1.5 s is below gtc
    assert ps.file_counts([[(1.5, 2.5)]], [[d]]) == [[1, 0, 0]]            # 0.5 of 1.0 s: exactly gtc
    # class 0's detection misses class 0 and covers 0.25 of itself with class 1's ground truth: a cross-trigger at cttc 0.25
    ref, est = [[(5.0, 6.0)], [(1.75, 4.0)]], [[(1.0, 2.0)], []]
    assert ps.file_counts(ref, est, cttc=0.25) == [[0, 1, 0, 1], [0, 0, 0, 0]]
    assert ps.file_counts(ref, est, cttc=0.25 + eps) == [[0, 1, 0, 0], [0, 0, 0, 0]]
    # zero-length events fail every test, even at threshold 0
    assert ps.file_counts([[(1.0, 1.0)]], [[(1.0, 1.0)]], dtc=0.0, gtc=0.0, cttc=0.0) == [[0, 1, 0]]

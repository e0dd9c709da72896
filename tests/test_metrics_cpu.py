"""CPU-side checks of dcase2019_task4_amd.metrics: the packing of annotation tables into the arrays sed_event_counts reads,
the ratio formulas on hand-written counts, and the numpy / scipy statement of the definitions (tests/sed_eval_np.py) on hand
cases - the statement the device code is pinned to in tests/test_gpu_metrics.py."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

from tests import sed_eval_np as se


def _df(rows):
    return pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])


def test_ref_events_packing_order_nan_files_absent_files_and_overlaps():
    from dcase2019_task4_amd.metrics import RefEvents
    nan = float("nan")
    df = _df([("b.wav", 4.0, 5.0, "dog"), ("a.wav", 2.0, 3.0, "cat"), ("b.wav", 1.0, 2.5, "dog"),
              ("c.wav", nan, nan, nan),                       # a file without events: one NaN-label row
              ("b.wav", 1.2, 2.0, "dog"),                     # overlaps the event above, same class
              ("b.wav", 0.5, 0.7, "cat"), ("zzz.wav", 0.0, 1.0, "cat")])       # a file that is not evaluated
    files, labels = ["c.wav", "b.wav", "absent.wav", "a.wav"], ["cat", "dog", "bird"]
    ref = RefEvents.from_dataframe(df, files, labels, device="cpu")
    assert len(ref) == 4 and ref.nclass == 3 and ref.max_per_column == 3
    ptr = ref.ptr.numpy()
    assert ptr.dtype == np.int32 and ptr.shape == (4 * 3 + 1,)
    #            c.wav      b.wav (cat, dog, bird)   absent     a.wav
    assert ptr.tolist() == [0, 0, 0, 0, 1, 4, 4, 4, 4, 4, 5, 5, 5]
    assert ref.onset.dtype == torch.float64
    np.testing.assert_array_equal(ref.onset.numpy()[:5], [0.5, 1.0, 1.2, 4.0, 2.0])      # sorted by onset inside a column
    np.testing.assert_array_equal(ref.offset.numpy()[:5], [0.7, 2.5, 2.0, 5.0, 3.0])
    # an empty table, and a label outside the list
    empty = RefEvents.from_dataframe(_df([]), files, labels, device="cpu")
    assert empty.ptr.numpy().tolist() == [0] * 13 and empty.max_per_column == 0
    with pytest.raises(ValueError):
        RefEvents.from_dataframe(_df([("a.wav", 0.0, 1.0, "cow")]), files, labels, device="cpu")
    with pytest.raises(ValueError):
        RefEvents.from_dataframe(df, ["a.wav", "a.wav"], labels, device="cpu")


def test_ref_events_on_a_cpu_device_refuses_to_score():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.metrics import RefEvents, event_counts, event_counts_from_events, weak_counts
    ref = RefEvents.from_dataframe(_df([("a.wav", 0.0, 1.0, "cat")]), ["a.wav"], ["cat"], device="cpu")
    with pytest.raises(_lib.SedError):
        event_counts(torch.zeros(1, 8, 1), ref)
    with pytest.raises(_lib.SedError):
        event_counts_from_events(ref, ref)
    with pytest.raises(_lib.SedError):
        weak_counts(torch.zeros(2, 3), torch.zeros(2, 3), [0.5] * 3)
    with pytest.raises(_lib.SedError):
        RefEvents.from_dataframe(_df([]), ["a.wav"], [f"c{i}" for i in range(17)], device="cpu")      # more than 16 classes


def test_event_metrics_from_hand_written_counts():
    from dcase2019_task4_amd.metrics import EventMetrics, SegmentMetrics
    #                     Ntp Nref Nsys
    counts = np.array([[3, 4, 6],          # P = 1/2, R = 3/4, F = 0.6
                       [0, 5, 0],          # Nsys == 0: P = 0 (zero_score), R = 0, F = 0
                       [0, 0, 2],          # Nref == 0: R = NaN, F = NaN - left out of the class-wise average
                       [0, 0, 0]])         # all-zero class: P = 0, R = NaN
    m = EventMetrics(["a", "b", "c", "d"], counts)
    cw = m.results_class_wise_metrics()
    assert cw["a"]["f_measure"] == {"f_measure": pytest.approx(0.6, rel=1e-15), "precision": 0.5, "recall": 0.75}
    assert cw["a"]["error_rate"] == {"error_rate": 1.0, "deletion_rate": 0.25, "insertion_rate": 0.75}
    assert cw["a"]["count"] == {"Nref": 4, "Nsys": 6}
    assert cw["b"]["f_measure"] == {"f_measure": 0.0, "precision": 0.0, "recall": 0.0}
    assert cw["b"]["error_rate"]["error_rate"] == 1.0
    assert cw["c"]["f_measure"]["precision"] == 0.0 and math.isnan(cw["c"]["f_measure"]["recall"])
    assert math.isnan(cw["c"]["f_measure"]["f_measure"]) and math.isnan(cw["c"]["error_rate"]["error_rate"])
    assert cw["d"]["f_measure"]["precision"] == 0.0 and math.isnan(cw["d"]["f_measure"]["f_measure"])
    av = m.results_class_wise_average_metrics()
    assert av["f_measure"]["f_measure"] == (2 * 0.5 * 0.75 / (0.5 + 0.75) + 0.0) / 2          # nanmean over a, b
    assert av["f_measure"]["precision"] == 0.125 and av["f_measure"]["recall"] == 0.375
    assert av["error_rate"]["error_rate"] == 1.0
    assert av["f_measure"]["f_measure"] == se.class_wise_average_f(counts)
    ov = m.results_overall_metrics()
    assert ov["f_measure"]["precision"] == 3 / 8 and ov["f_measure"]["recall"] == 3 / 9
    assert ov["f_measure"]["f_measure"] == 2 * (3 / 8) * (3 / 9) / (3 / 8 + 3 / 9)
    assert math.isnan(ov["error_rate"]["error_rate"])               # needs a label-agnostic matching: not provided
    assert set(m.results()) == {"overall", "class_wise", "class_wise_average"}
    assert "Event based" in str(m) and "Class-wise average" in str(m)
    # every class without references: the average is NaN, not an exception
    assert math.isnan(EventMetrics(["a"], [[0, 0, 3]]).results_class_wise_average_metrics()["f_measure"]["f_measure"])
    #                               Ntp Nfp Nfn Ntn
    s = SegmentMetrics(["a", "b"], [[6, 2, 2, 10], [0, 0, 0, 20]])
    assert s.results_class_wise_metrics()["a"]["f_measure"] == {"f_measure": 0.75, "precision": 0.75, "recall": 0.75}
    assert s.results_class_wise_metrics()["a"]["count"] == {"Nref": 8, "Nsys": 8}
    assert s.results_class_wise_average_metrics()["f_measure"]["f_measure"] == 0.75 and s.Ntn == {"a": 10, "b": 20}
    assert "Segment based" in str(s)


def test_operating_points_broadcast_and_limits():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.metrics import operating_points
    thr, win = operating_points((0.3, 0.5, 0.7), (5,), device="cpu")
    assert thr.dtype == torch.float32 and win.dtype == torch.int32 and win.tolist() == [5, 5, 5]
    assert thr.numpy().tolist() == [np.float32(0.3), np.float32(0.5), np.float32(0.7)]
    with pytest.raises(ValueError):
        operating_points((0.3, 0.5), (1, 5, 9), device="cpu")
    with pytest.raises(_lib.SedError):
        operating_points((0.5,), (64,), device="cpu")


def test_helper_optimal_matching_beats_first_fit_on_the_hand_case():
    ref, est = [(1.0, 2.0), (1.15, 2.15)], [(1.1, 2.1), (0.85, 1.85)]
    assert se.hit_matrix(ref, est).tolist() == [[True, True], [True, False]]
    assert se.optimal_ntp(ref, est) == 2 and se.first_fit_ntp(ref, est) == 1
    # the same failure with both lists sorted by onset, as the packed arrays hold them
    ref, est = [(1.0, 2.0), (1.05, 2.4)], [(0.9, 2.15), (1.0, 1.9)]
    assert se.optimal_ntp(ref, est) == 2 and se.first_fit_ntp(ref, est) == 1
    assert se.optimal_ntp([], est) == 0 and se.optimal_ntp(ref, []) == 0


def test_helper_collar_is_inclusive_and_offset_tolerance_grows_with_length():
    assert se.optimal_ntp([(1.0, 2.0)], [(1.0 + 0.2, 2.0)]) == 1            # |d onset| == t_collar exactly (1.2 - 1.0 <= 0.2 in fp64)
    assert math.fabs(1.0 - (1.0 + 0.2)) <= 0.2
    assert se.optimal_ntp([(1.0, 2.0)], [(0.5 + 0.2 + 0.5, 2.0)]) == 1 and se.optimal_ntp([(1.0, 2.0)], [(1.25, 2.0)]) == 0
    assert se.optimal_ntp([(0.25, 1.0)], [(0.0, 1.0)], t_collar=0.25) == 1 and se.optimal_ntp([(0.25, 1.0)], [(0.0, 1.0)]) == 0
    assert se.optimal_ntp([(0.0, 10.0)], [(0.0, 8.0)]) == 1                 # 20 % of 10 s
    assert se.optimal_ntp([(0.0, 10.0)], [(0.0, 7.9)]) == 0
    assert se.optimal_ntp([(0.0, 0.5)], [(0.0, 0.7)]) == 1                  # short event: the collar, not 20 % of 0.5 s
    assert se.optimal_ntp([(0.0, 0.5)], [(0.0, 0.75)]) == 0


def test_helper_segment_counts():
    #          class 0                      class 1
    ref = [[(0.5, 2.0), (1.5, 2.5)], []]                 # segments 0, 1, 2
    est = [[(1.0, 1.2)], [(3.0, 4.2)]]                   # segment 1 / segments 3, 4: the file has ceil(4.2) = 5 segments
    ev, seg = se.file_counts(ref, est)
    assert ev.tolist() == [[0, 2, 1], [0, 0, 1]]
    assert seg.tolist() == [[1, 0, 2, 2], [0, 2, 0, 3]]
    ev, seg = se.file_counts([[], []], [[], []])
    assert seg.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]
    _, seg = se.file_counts([[(0.0, 1.0)]], [[(0.0, 1.0)]], res=0.5)
    assert seg.tolist() == [[2, 0, 0, 0]]


def test_synthetic_references_separate_optimal_from_first_fit_and_stay_inside_the_limit():
    """The facts tests/test_gpu_metrics.py relies on, checked where no GPU is needed."""
    from oracle import postprocess_np as pp
    from oracle import synth
    files, labels = [f"clip_{i}.wav" for i in range(64)], [f"c{i}" for i in range(10)]
    for T in (78, 108):
        post = synth.make_posteriors(1, 64, T).numpy()
        est = se.columns_from_rows(pp.predictions(post, files, labels, 8, 44100, 511, 0.5, 5), files, labels)
        dec7 = se.columns_from_rows(pp.predictions(post, files, labels, 8, 44100, 511, 0.5, 7), files, labels)
        ref = se.jittered_references(dec7, np.random.RandomState(7))
        pairs = [(r, e) for rf, ef in zip(ref, est) for r, e in zip(rf, ef)]
        assert sum(se.optimal_ntp(r, e) for r, e in pairs) > sum(se.first_fit_ntp(r, e) for r, e in pairs)
        assert max(max(len(r), len(e)) for r, e in pairs) <= 64

"""CPU-side checks of the overall error rate with substitutions: the statement of its definition (tests/error_rate_np.py) on
hand cases and random small files, the ratio formulas of ``EventMetrics`` / ``SegmentMetrics(overall=...)``, and what
tests/test_gpu_error_rate.py relies on about its own inputs (tests/error_rate_cases.py)."""
import math

import numpy as np
import pytest

from dcase2019_task4_amd.metrics import ErrorCounts, EventMetrics, SegmentMetrics      # the feature under test
from tests import error_rate_cases as ec
from tests import error_rate_np as er
from tests import long_score_np as ls
from tests import sed_eval_np as se


# ---- hand cases ---------------------------------------------------------------------------------------------------------------
def test_a_pure_substitution_is_one_error_not_two():
    ref, est = [[(1.0, 2.0)], []], [[], [(1.0, 2.0)]]              # the same interval under another label
    assert er.event_overall(ref, est) == (1, 1, 1) and er.n_tp(ref, est) == 0
    assert er.segment_overall(ref, est) == (1, 0, 0)
    from dcase2019_task4_amd.metrics import EventMetrics, SegmentMetrics
    ev, seg = se.file_counts(ref, est)
    e = EventMetrics(["a", "b"], ev, overall=er.event_overall(ref, est)).results_overall_metrics()["error_rate"]
    assert e == {"error_rate": 1.0, "substitution_rate": 1.0, "deletion_rate": 0.0, "insertion_rate": 0.0}
    s = SegmentMetrics(["a", "b"], seg, overall=er.segment_overall(ref, est)).results_overall_metrics()["error_rate"]
    assert s == {"error_rate": 1.0, "substitution_rate": 1.0, "deletion_rate": 0.0, "insertion_rate": 0.0}
    # among three references: ER = 1 / Nref
    ref = [[(1.0, 2.0), (4.0, 5.0)], [(7.0, 8.0)]]
    est = [[(4.0, 5.0)], [(7.0, 8.0), (1.0, 2.0)]]
    nref, nsys, nany = er.event_overall(ref, est)
    assert (nref, nsys, nany, er.n_tp(ref, est)) == (3, 3, 3, 2)
    m = EventMetrics(["a", "b"], se.file_counts(ref, est)[0], overall=(nref, nsys, nany))
    assert m.results_overall_metrics()["error_rate"] == {"error_rate": 1 / 3, "substitution_rate": 1 / 3, "deletion_rate": 0.0,
                                                         "insertion_rate": 0.0}


def test_a_same_label_hit_is_not_counted_again():
    ref, est = [[(1.0, 2.0)], []], [[(1.05, 2.0)], [(1.0, 2.1)]]   # the hit, and a second detection of another class on it
    assert er.n_tp(ref, est) == 1 and er.event_overall(ref, est) == (1, 2, 1)          # Nsubs = 0, one insertion
    assert er.greedy_nsubs(ref, est) == 0
    assert er.segment_overall(ref, est) == (0, 0, 2)               # class b active in segments 1 and 2, nothing missed


def test_a_tie_where_the_greedy_pass_finds_fewer_than_nany():
    """Leftover references r1, r2 of class a; leftover estimated events x of class b and y of class c.  r1 is compatible with x
    and y, r2 with x only.  In (class, onset) order the greedy pass gives x to r1 and leaves r2 alone; the maximum matching
    pairs r1 - y and r2 - x."""
    ref = [[(1.0, 2.0), (1.2, 2.0)], [], []]
    est = [[], [(1.1, 2.0)], [(0.85, 2.0)]]
    assert er.time_compatible(ref[0][0], est[1][0]) and er.time_compatible(ref[0][0], est[2][0])
    assert er.time_compatible(ref[0][1], est[1][0]) and not er.time_compatible(ref[0][1], est[2][0])
    assert er.n_tp(ref, est) == 0 and er.event_overall(ref, est) == (2, 2, 2)
    assert er.greedy_nsubs(ref, est) == 1                           # sed_eval's count here: ER = (1 + 1 + 1) / 2, ours 2 / 2


def test_empty_sides_and_no_reference():
    from dcase2019_task4_amd.metrics import EventMetrics, SegmentMetrics
    none = [[], []]
    some = [[(0.5, 1.5)], [(3.0, 3.5)]]
    assert er.event_overall(none, none) == (0, 0, 0) and er.segment_overall(none, none) == (0, 0, 0)
    assert er.event_overall(some, none) == (2, 0, 0) and er.segment_overall(some, none) == (0, 3, 0)
    assert er.event_overall(none, some) == (0, 2, 0) and er.segment_overall(none, some) == (0, 0, 3)
    ev, seg = se.file_counts(none, some)
    for m in (EventMetrics(["a", "b"], ev, overall=(0, 2, 0)), SegmentMetrics(["a", "b"], seg, overall=(0, 0, 3))):
        assert all(math.isnan(v) for v in m.results_overall_metrics()["error_rate"].values())     # Nref = 0
    assert all(math.isnan(v) for v in er.rates(0, 0, 0, 3))
    ev, seg = se.file_counts(some, none)
    assert EventMetrics(["a", "b"], ev, overall=(2, 0, 0)).results_overall_metrics()["error_rate"]["deletion_rate"] == 1.0
    assert SegmentMetrics(["a", "b"], seg, overall=(0, 3, 0)).results_overall_metrics()["error_rate"]["error_rate"] == 1.0


# ---- random small files -------------------------------------------------------------------------------------------------------
def test_inequalities_and_identities_on_random_small_files():
    rs = np.random.RandomState(3)
    strict = subs = 0
    for trial in range(300):
        nclass = int(rs.randint(1, 5))
        ref = [sorted((float(a), float(a + l)) for a, l in zip(rs.uniform(0, 4, size=rs.randint(0, 5)),
                                                                   rs.uniform(0.05, 2.0, size=8))) for _ in range(nclass)]
        est = ec.estimate_of(ref, rs, nclass, 4.0, p_relabel=0.5)
        nref, nsys, nany = er.event_overall(ref, est)
        ntp = er.n_tp(ref, est)
        assert ntp <= nany <= min(nref, nsys)
        greedy = er.greedy_nsubs(ref, est)
        assert greedy <= nany - ntp
        strict += greedy < nany - ntp
        subs += nany - ntp
        # Nany is the label-wise Ntp of the same events under ONE label
        (r1,), (e1,) = ec.one_class([ref]), ec.one_class([est])
        assert nany == se.optimal_ntp(r1[0], e1[0])
        _, seg = se.file_counts(ref, est)
        S, D, I = er.segment_overall(ref, est)
        assert S + D == seg[:, 2].sum() and S + I == seg[:, 1].sum() and min(S, D, I) >= 0
        if nclass == 1:
            assert nany == ntp and S == 0
    assert subs > 100 and strict > 0                                # the files do hold substitutions, and greedy does lose some


# ---- the metrics objects ------------------------------------------------------------------------------------------------------
def test_metrics_with_overall_on_hand_written_counts_and_unchanged_without():
    from dcase2019_task4_amd.metrics import EventMetrics, SegmentMetrics
    #                     Ntp Nref Nsys
    counts = np.array([[3, 4, 6], [0, 5, 0], [0, 0, 2]])
    plain = EventMetrics(["a", "b", "c"], counts)
    m = EventMetrics(["a", "b", "c"], counts, overall=(9, 8, 5))     # Nany = 5: Nsubs 2, Nfn 4, Nfp 3
    e = m.results_overall_metrics()["error_rate"]
    assert e == {"error_rate": 9 / 9, "substitution_rate": 2 / 9, "deletion_rate": 4 / 9, "insertion_rate": 3 / 9}
    assert m.results_overall_metrics()["f_measure"] == plain.results_overall_metrics()["f_measure"]
    assert repr(m.results_class_wise_metrics()) == repr(plain.results_class_wise_metrics())          # (repr: NaN entries)
    assert "Overall error rate: ER  1.00  S  0.22  D  0.44  I  0.33" in str(m)
    assert "Overall error rate" not in str(plain) and str(m).replace(str(m).split("\n")[2] + "\n", "") == str(plain)
    assert all(math.isnan(v) for v in plain.results_overall_metrics()["error_rate"].values())
    assert set(plain.results_overall_metrics()["error_rate"]) == set(e)
    for bad in ((9, 8, 2), (9, 8, 9), (8, 8, 5), (9, 7, 5)):        # Nany < Ntp, > min(Nref, Nsys); foreign Nref / Nsys
        with pytest.raises(ValueError):
            EventMetrics(["a", "b", "c"], counts, overall=bad)
    #                               Ntp Nfp Nfn Ntn
    seg = [[6, 2, 2, 10], [0, 3, 1, 16]]                            # Nref 9, sum Nfn 3, sum Nfp 5
    s = SegmentMetrics(["a", "b"], seg, overall=(2, 1, 3))
    assert s.results_overall_metrics()["error_rate"] == {"error_rate": 6 / 9, "substitution_rate": 2 / 9,
                                                         "deletion_rate": 1 / 9, "insertion_rate": 3 / 9}
    assert "Overall error rate: ER  0.67" in str(s)
    plain_s = SegmentMetrics(["a", "b"], seg)
    assert all(math.isnan(v) for v in plain_s.results_overall_metrics()["error_rate"].values())
    assert s.results_class_wise_average_metrics() == plain_s.results_class_wise_average_metrics() and s.Ntn == plain_s.Ntn
    with pytest.raises(ValueError):
        SegmentMetrics(["a", "b"], seg, overall=(2, 2, 3))          # S + D != sum Nfn
    with pytest.raises(ValueError):
        SegmentMetrics(["a", "b"], seg, overall=(4, -1, 1))


def test_the_binding_declares_the_new_entry_points_and_cpu_devices_are_refused():
    import torch
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd import metrics as M
    for name in ("sed_error_counts", "sed_long_error_counts", "sed_long_sweep_error_counts", "sed_long_error_ws_bytes",
                 "sed_long_sweep_error_ws_bytes"):
        assert name in _lib.exported_symbols()
    l = _lib.lib()
    assert l.sed_long_error_ws_bytes(1000, 1000, 3, 3) > l.sed_long_score_ws_bytes(1000, 1000, 3, 3)
    assert l.sed_long_error_ws_bytes(1000, 1000, 3, 17) == 0 and l.sed_long_sweep_error_ws_bytes(10, 10, 1, 1, 0) == 0
    # the reference side is merged ONCE: what K points add to the workspace does not depend on the reference events
    grow = [l.sed_long_sweep_error_ws_bytes(5000, r, 3, 4, 9) - l.sed_long_sweep_error_ws_bytes(5000, r, 3, 4, 1)
            for r in (0, 1000, 100000)]
    assert grow[0] == grow[1] == grow[2] > 0
    empty = ErrorCounts(2, 3, "cpu")                                 # the accumulator itself needs no GPU
    assert empty.ev.shape == (2, 3) and empty.seg.shape == (2, 3) and all((a == 0).all() for a in empty.host())
    ref = M.RefEvents(np.zeros(2, np.int32), [], [], ["a.wav"], ["cat"], device="cpu")
    for call in (lambda: M.error_counts(torch.zeros(1, 8, 1), ref), lambda: M.error_counts_from_events(ref, ref),
                 lambda: M.long_error_from_events(ref, ref), lambda: M.long_sweep_error_from_events([ref, ref], ref)):
        with pytest.raises(_lib.SedError):
            call()


# ---- what the device tests rely on about their inputs -------------------------------------------------------------------------
def _within(ref, est, limit=64):
    sizes = [er.merged_cluster_sizes(r, e) for r, e in zip(ref, est)]
    assert max(max(s) for s in sizes) <= limit, sizes
    return max(max(s) for s in sizes)


@pytest.mark.parametrize("nclass", ec.CLIP_CLASSES)
def test_clip_cases_stay_within_the_limits_and_hold_what_they_are_for(nclass):
    ref, est = ec.clip_events(nclass)
    _within(ref, est)
    assert max(len(c) for side in (ref, est) for f in side for c in f) <= 64
    assert not any(ref[1]) and not any(est[1])                                           # the empty clip
    assert min(on for f in ref for c in f for on, _ in c) < 0.0                          # an onset before 0
    last = lambda f: max(math.ceil(off) for c in f for _, off in c)
    assert last(est[0]) > last(ref[0])                                                   # the sides end in different segments
    ev_o, seg_o = er.set_overall(ref, est)
    if nclass > 1:
        assert seg_o[:, 0].sum() > 0 and (ev_o[:, 2].sum() - sum(er.n_tp(r, e) for r, e in zip(ref, est))) > 0
    post, dref, dests = ec.decoded_case(nclass)
    assert post.shape == (ec.N_CLIPS, ec.T, nclass) and dests[0] != dests[1]
    for dest in dests:
        _within(dref, dest)
        assert max(len(c) for side in (dref, dest) for f in side for c in f) <= 64
        assert not any(dest[1]) and sum(len(c) for f in dest for c in f) > nclass
    # relabelled to one class these clips still fit the class-wise clip call: the device test uses it on all of them
    for cols in (ref, est, dref, dests[0]):
        assert max(len(f[0]) for f in ec.one_class(cols)) <= 64


def test_the_chain_cases_are_one_merged_cluster_of_64_and_of_65():
    ref, est = ec.chain_case(64)
    assert er.merged_cluster_sizes(ref[1], est[1]) == (64, 64)
    assert max(len(c) for side in (ref[1], est[1]) for c in side) <= 5
    assert er.event_overall(ref[1], est[1])[2] == 64
    for n_ref, n_est, want in ((65, 64, (65, 64)), (64, 65, (64, 65))):
        ref, est = ec.chain_case(n_ref, n_est)
        assert er.merged_cluster_sizes(ref[1], est[1]) == want
        assert max(len(c) for side in (ref, est) for f in side for c in f) <= 64         # no COLUMN is over the limit
        _within([ref[0], ref[2]], [est[0], est[2]])


def test_long_cases_stay_within_the_limits_and_the_straddling_cluster_straddles():
    tile = 64
    ref, est = ec.long_events(tile)
    biggest = _within(ref, est)
    assert biggest >= 6
    assert len(ref[0][0]) == 300 and not any(ref[1]) and not any(est[1]) and not ref[0][1] and not ref[0][2] and not ref[2][2]
    assert {on for on, _ in ref[0][3]} <= {on for on, _ in ref[0][0]}                    # equal onsets across classes
    assert any(first < tile < first + n for first, n, _ in er.merged_clusters(ref[2], est[2]))
    assert all(not ls.decreasing(c) for side in (ref, est) for f in side for c in f)
    ev_o, _ = er.set_overall(ref, est)
    assert ev_o[:, 2].sum() - sum(er.n_tp(r, e) for r, e in zip(ref, est)) > 10          # substitutions
    for K in (1, 9):
        _, ests = ec.sweep_events(K, tile)
        for e in ests:
            _within(ref, e)
            assert all(not ls.decreasing(c) for f in e for c in f)
    ptr, pairs, cols = ec.frame_table()
    refs = ec.frame_references(cols)
    _within(refs, cols)
    assert max(len(c) for f in cols for c in f) == 400 and ptr[-1] == len(pairs)
    assert all(not ls.decreasing(c) for side in (refs, cols) for f in side for c in f)

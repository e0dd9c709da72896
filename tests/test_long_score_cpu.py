"""CPU checks of the long-recording scoring: the cluster rule of tests/long_score_np.py against the global matching of
tests/sed_eval_np.py, the cluster sizes of every column the GPU tests score (they must stay within 64 per side, or a GPU test
would rest on an error path), and the C-ABI declarations."""
import os
import re

import numpy as np
import pytest

from dcase2019_task4_amd import _lib
from tests import long_score_np as ls
from tests import sed_eval_np as se

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64                                                             # sed_long_tile_events(); test_gpu_long_score checks it


def test_header_declares_the_long_scoring_calls_and_the_binding_knows_them():
    src = open(os.path.join(REPO, "include", "dcase_sed.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("sed_long_event_counts", "sed_long_psds_counts", "sed_long_score_ws_bytes", "sed_long_tile_events"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.exported_symbols(), name
    for word in ("valid", "cluster", "bit 64", "zero terms"):
        assert word in src.lower(), word


def test_python_entry_points_exist_and_refuse_the_cpu():
    from dcase2019_task4_amd import metrics
    from dcase2019_task4_amd.longrec import LongRecordingSet
    for name in ("long_event_counts", "long_psds_counts", "long_event_counts_from_events", "long_psds_counts_from_events",
                 "validate_long"):
        assert callable(getattr(metrics, name)), name
    assert callable(LongRecordingSet.durations)
    ptr, on, off = ls.pack([[[(0.0, 1.0)], []]])
    ref = metrics.RefEvents(ptr, on, off, ["a"], ["x", "y"], device="cpu")
    assert ref.ptr64.dtype.is_floating_point is False and ref.ptr64.element_size() == 8
    with pytest.raises(_lib.SedError):
        metrics.long_event_counts_from_events(ref, ref)
    with pytest.raises(_lib.SedError):
        metrics.long_psds_counts_from_events(ref, ref)
    assert "cluster" in metrics._LONG_ERR_BITS[1] and "cluster" in metrics._LONG_ERR_BITS[2] and 64 in metrics._LONG_ERR_BITS
    assert metrics._ERR_BITS[1] == "a (file, class) column has more than 64 reference events"      # the clip wording stays


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_cluster_sum_equals_the_global_matching_on_burst_columns(seed):
    """~900 events per side; the largest cluster stays within one burst of at most 60, and greedy matching is wrong here."""
    ref, est = ls.burst_column(np.random.RandomState(seed))
    assert 700 <= len(ref) <= 1100 and 700 <= len(est) <= 1100
    nr, ne = ls.cluster_sizes(ref, est)
    assert 40 <= nr <= 60 and 40 <= ne <= 60
    want = se.optimal_ntp(ref, est)
    assert ls.cluster_ntp(ref, est) == want
    assert se.first_fit_ntp(ref, est) < want and se.first_fit_ntp(ref, est, est_major=True) < want


def test_cluster_sum_equals_the_global_matching_on_the_other_builders():
    rs = np.random.RandomState(3)
    cases = [ls.spaced_column(rs, n) for n in (0, 1, 64, 65, 200)] + [ls.tile_edge_column(rs, TILE, n) for n in (64, 65, 133)]
    cases += [ls.chained_pair(20, 0.0), ls.chained_pair(20, np.spacing(1.0))]
    flicker = [(k / 2.0, k / 2.0 + 0.25) for k in range(300)]           # on for a quarter second, twice a second
    cases.append((flicker, [(a + 0.01, b) for a, b in flicker]))
    for ref, est in cases:
        tc = 0.25 if len(ref) == 40 else 0.2
        assert ls.cluster_ntp(ref, est, tc) == se.optimal_ntp(ref, est, tc)
    assert ls.cluster_sizes(*cases[-1]) == (1, 1)                     # a flicker: clusters of one


def test_tile_edge_columns_have_a_cluster_across_the_edge():
    ref, est = ls.tile_edge_column(np.random.RandomState(4), TILE, 2 * TILE + 5)
    spans = [(min(r), max(r)) for r, _ in ls.clusters(ref, est) if r]
    assert any(lo < TILE <= hi for lo, hi in spans) and any(lo < 2 * TILE <= hi for lo, hi in spans)


def test_boundary_pairs_cut_exactly_one_ulp_beyond_the_collar():
    """Dyadic onsets: exactly t_collar apart is compatible and not cut (one cluster of 2n), one ulp more is cut."""
    n = 40
    ref, est = ls.chained_pair(n, 0.0)
    assert ref[n][0] - est[n - 1][0] == 0.25 and ls.cluster_sizes(ref, est, 0.25) == (2 * n, 2 * n)
    ulp = np.spacing(ref[n][0])
    ref, est = ls.chained_pair(n, float(ulp))
    assert ref[n][0] - est[n - 1][0] > 0.25 and ls.cluster_sizes(ref, est, 0.25) == (n, n)
    assert ls.expected_err([[ref]], [[est]], 0.25) == 0
    assert ls.expected_err([[ls.chained_pair(n, 0.0)[0]]], [[ls.chained_pair(n, 0.0)[1]]], 0.25) == 3


def test_every_column_the_gpu_tests_score_has_clusters_within_64():
    sets = [ls.main_columns(TILE, seed) for seed in (0,)]
    sets += [ls.small_columns(3, 1, 11), ls.small_columns(3, 16, 12), ls.small_columns(3, 3, 13, n_max=50)]
    for ref_cols, est_cols in sets:
        assert ls.expected_err(ref_cols, est_cols) == 0
        for r_file, e_file in zip(ref_cols, est_cols):
            for r, e in zip(r_file, e_file):
                nr, ne = ls.cluster_sizes(r, e)
                assert nr <= 64 and ne <= 64
    ref_cols, est_cols = ls.main_columns(TILE, 0)
    lengths = [len(c) for f in ref_cols for c in f]
    assert lengths[:4] == [0, 1, 64, 65] and lengths[5:] == [TILE - 1, TILE, TILE + 1, 2 * TILE + 5] and lengths[4] > 700
    assert ls.cluster_sizes(ref_cols[1][1], est_cols[1][1])[0] > 50   # the burst column: large clusters, yet within the limit
    small_ref, small_est = ls.small_columns(3, 3, 13, n_max=50)
    assert max(len(c) for f in small_ref + small_est for c in f) <= 64         # clip-sized: the clip kernels score it too


def test_the_frames_mode_columns_have_clusters_within_64():
    est_cols = ls.stitch_columns(ls.stitch_patterns(ls.stitch_lengths(512)), 8.0, 44100 / 511)
    ref_cols = ls.sorted_jittered_references(est_cols, 5)
    assert max(len(c) for f in est_cols for c in f) > 200
    assert ls.expected_err(ref_cols, est_cols) == 0
    for r_file, e_file in zip(ref_cols, est_cols):
        for r, e in zip(r_file, e_file):
            assert ls.cluster_ntp(r, e) == se.optimal_ntp(r, e)


def test_error_inputs_raise_exactly_their_bit_in_the_cluster_statement():
    inside = [(1.0 + k / 1024.0, 2.0) for k in range(65)]
    one = [(1.01, 2.0)]
    assert ls.expected_err([[inside]], [[one]]) == 1
    assert ls.expected_err([[one]], [[inside]]) == 2
    assert ls.expected_err([[[(2.0, 3.0), (1.0, 1.5)]]], [[one]]) == 64
    assert ls.expected_err([[[(1.0, 65536.5)]]], [[one]]) == 4
    assert ls.expected_err([[[(1.0, 65536.0)]]], [[one]]) == 0

"""-m gpu tests of the long-recording scoring: sed_long_event_counts / sed_long_psds_counts exact against tests/sed_eval_np.py
and tests/psds_np.py on columns of hundreds of events (lengths at the tile edges, clusters across them, a ~900-event burst
column on which greedy matching is wrong), the collar boundary, agreement with the clip kernels, the frames mode on
sed_stitch_decode's table, validate_long end to end, every error bit alone, sentinels, reproducibility and graph replay.
tests/test_long_score_cpu.py checks that no scored column here holds a cluster of more than 64 events per side."""
import functools

import numpy as np
import pytest
import torch

from tests import gpu_util as gu
from tests import long_score_np as ls
from tests import psds_np
from tests import sed_eval_np as se
from tests.long_util import SENT, ScoreCall, _ref_events, _Scaler, _stitch_inputs

pytestmark = pytest.mark.gpu

def _tile():
    from dcase2019_task4_amd import _lib
    return int(_lib.lib().sed_long_tile_events())


@functools.lru_cache(maxsize=None)
def _case(name):
    """(ref_cols, est_cols, ev, seg, ps): the columns and the oracle's per-column counts, computed once."""
    if name == "main":
        ref, est = ls.main_columns(_tile(), 0)
    elif name == "nc1":
        ref, est = ls.small_columns(3, 1, 11)
    elif name == "nc16":
        ref, est = ls.small_columns(3, 16, 12)
    else:
        ref, est = ls.small_columns(3, 3, 13, n_max=50)
    ev, seg = se.set_counts(ref, est)
    return ref, est, ev, seg, np.array(psds_np.set_counts(ref, est))


def _check_all(got, ev, seg, ps, events=True, psds=True):
    assert got["err"] == 0
    if events:
        np.testing.assert_array_equal(got["ev"], ev)
        np.testing.assert_array_equal(got["seg"], seg)
        np.testing.assert_array_equal(got["ev_t"], ev.sum(0))
        np.testing.assert_array_equal(got["seg_t"], seg.sum(0))
    if psds:
        np.testing.assert_array_equal(got["ps"], ps)
        np.testing.assert_array_equal(got["ps_t"], ps.sum(0))


# ---- exact agreement, given events -------------------------------------------------------------------------------------------------
def test_tile_accessor_and_workspace_size():
    from dcase2019_task4_amd import _lib
    l = _lib.lib()
    assert _tile() == 64
    assert l.sed_long_score_ws_bytes(1000, 1000, 3, 3) > 0 and l.sed_long_score_ws_bytes(0, 0, 1, 1) > 0
    assert l.sed_long_score_ws_bytes(1000, 1000, 3, 17) == 0 and l.sed_long_score_ws_bytes(-1, 0, 1, 1) == 0
    assert l.sed_long_score_ws_bytes(1 << 31, 0, 1, 1) == 0 and l.sed_long_score_ws_bytes(10, 10, 0, 1) == 0


@pytest.mark.parametrize("name", ["main", "nc1", "nc16"])
def test_given_events_are_exact_and_two_runs_identical(name):
    """main: 3 x 3 columns of 0, 1, 64, 65, ~900 (bursts), tile - 1, tile, tile + 1 and 2 tile + 5 reference events, with
    clusters across tile edges, zero-length events, overlapping references and detections over other classes' references."""
    ref, est, ev, seg, ps = _case(name)
    raw = ScoreCall(ls.pack(est), ls.pack(ref), len(ref), len(ref[0]))
    a = raw.run()
    _check_all(a, ev, seg, ps)
    if name == "main":
        assert ev[1, 1, 1] > 700 and ev[1, 1, 0] > 250                         # the burst column was matched, not skipped
        assert se.first_fit_ntp(ref[1][1], est[1][1]) < ev[1, 1, 0]
        assert ps[:, :, 2:].sum() > 0 and ps[:, :, 0].sum() > 0
    b = raw.run()
    for k in ("ev", "seg", "ps", "ev_t", "seg_t", "ps_t"):
        assert a[k].tobytes() == b[k].tobytes(), k
    # totals accumulate; NULL per-column outputs
    raw.fill()
    assert raw.launch_events(columns=False) == 0 and raw.launch_events(columns=False) == 0
    assert raw.launch_psds(columns=False) == 0
    c = raw.get()
    np.testing.assert_array_equal(c["ev_t"], 2 * ev.sum(0))
    np.testing.assert_array_equal(c["seg_t"], 2 * seg.sum(0))
    np.testing.assert_array_equal(c["ps_t"], ps.sum(0))
    assert (c["ev"] == SENT).all() and (c["ps"] == SENT).all()


def test_other_criteria_and_resolutions():
    ref, est, _, _, _ = _case("small")
    for kw in (dict(t_collar=0.5, percentage_of_length=0.5, res=0.25), dict(t_collar=0.0, percentage_of_length=0.0, res=7.0)):
        ev, seg = se.set_counts(ref, est, **kw)
        got = ScoreCall(ls.pack(est), ls.pack(ref), 3, 3).run(psds=False, t_collar=kw["t_collar"], pct=kw["percentage_of_length"],
                                                         res=kw["res"])
        _check_all(got, ev, seg, None, psds=False)
    for kw in (dict(dtc=0.1, gtc=0.1, cttc=0.1), dict(dtc=1.0, gtc=0.9, cttc=0.0)):
        ps = np.array(psds_np.set_counts(ref, est, **kw))
        _check_all(ScoreCall(ls.pack(est), ls.pack(ref), 3, 3).run(events=False, **kw), None, None, ps, events=False)


# ---- the collar boundary -------------------------------------------------------------------------------------------------------------
def test_exactly_t_collar_apart_is_not_cut_and_one_ulp_more_is():
    """Dyadic onsets, t_collar = 0.25.  Two chains of 40 + 40 events joined by a pair exactly t_collar apart are ONE cluster of
    80 per side (bits 1 and 2: the pair was not cut); one ulp more and they are two clusters, scored exactly."""
    n = 40
    ref, est = ls.chained_pair(n, 0.0)
    got = ScoreCall(ls.pack([[est]]), ls.pack([[ref]]), 1, 1).run(psds=False, t_collar=0.25)
    assert got["err"] == 3 == ls.expected_err([[ref]], [[est]], 0.25)
    long_ref, long_est = ls.chained_pair(70, 0.0)                     # 140 per side: the cluster's end lies beyond the next tile
    assert ScoreCall(ls.pack([[long_est]]), ls.pack([[long_ref]]), 1, 1).run(psds=False, t_collar=0.25)["err"] == 3
    assert ls.expected_err([[long_ref]], [[long_est]], 0.25) == 3
    ref, est = ls.chained_pair(n, float(np.spacing(ref[n][0])))
    ev, seg = se.set_counts([[ref]], [[est]], t_collar=0.25)
    got = ScoreCall(ls.pack([[est]]), ls.pack([[ref]]), 1, 1).run(psds=False, t_collar=0.25)
    _check_all(got, ev, seg, None, psds=False)
    assert ev[0, 0, 0] == 2 * n
    # single pairs: compatible at exactly the collar, not one ulp beyond, on either side
    pairs_ref = [(1.0, 2.0), (11.0, 12.0), (21.0, 22.0), (31.0, 32.0)]
    pairs_est = [(1.25, 2.25), (10.75, 11.75), (float(np.nextafter(21.25, 99)), 22.0), (float(np.nextafter(30.75, 0)), 32.0)]
    ev, seg = se.set_counts([[pairs_ref]], [[pairs_est]], t_collar=0.25)
    assert ev[0, 0, 0] == 2
    got = ScoreCall(ls.pack([[pairs_est]]), ls.pack([[pairs_ref]]), 1, 1).run(psds=False, t_collar=0.25)
    _check_all(got, ev, seg, None, psds=False)


# ---- agreement with the clip kernels -------------------------------------------------------------------------------------------------
def test_clip_sized_columns_agree_with_the_clip_kernels():
    from dcase2019_task4_amd import metrics as M
    ref_cols, est_cols, ev, seg, ps = _case("small")
    ref, est = _ref_events(ref_cols), _ref_events(est_cols)
    assert max(ref.max_per_column, est.max_per_column) <= 64
    clip = M.event_counts_from_events(est, ref, per_column=True)
    clip_ps = M.psds_counts_from_events(est, ref, per_column=True)
    lng = M.long_event_counts_from_events(est, ref, per_column=True)
    lng_ps = M.long_psds_counts_from_events(est, ref, per_column=True)
    np.testing.assert_array_equal(lng.ev_columns.cpu().numpy(), clip.ev_columns[0].cpu().numpy())
    np.testing.assert_array_equal(lng.seg_columns.cpu().numpy(), clip.seg_columns[0].cpu().numpy())
    np.testing.assert_array_equal(lng_ps.columns.cpu().numpy(), clip_ps.columns[0].cpu().numpy())
    for a, b in zip(lng.host(), clip.host()):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(lng_ps.host(), clip_ps.host())
    np.testing.assert_array_equal(lng.ev_columns.cpu().numpy(), ev)
    # the clip kernels refuse what the long ones score
    big_ref, big_est, big_ev, _, _ = _case("main")
    with pytest.raises(Exception, match="more than 64"):
        M.event_counts_from_events(_ref_events(big_est), _ref_events(big_ref)).host()
    ev_l, _ = M.long_event_counts_from_events(_ref_events(big_est), _ref_events(big_ref), point=1).host()
    np.testing.assert_array_equal(ev_l[1], big_ev.sum(0))
    assert (ev_l[0] == 0).all()


# ---- frames mode -----------------------------------------------------------------------------------------------------------------------
NUM, DEN = 8.0, 44100 / 511


def _decoded_cols(ev_ptr, ev_pairs, n_rec, NC):
    """The host's doubles of a decoded table: cols[recording][class] = [(frame * num / den, ...)]."""
    return [[[(int(a) * NUM / DEN, int(b) * NUM / DEN) for a, b in ev_pairs[ev_ptr[r * NC + c]:ev_ptr[r * NC + c + 1]]]
             for c in range(NC)] for r in range(n_rec)]


_sorted_refs = ls.sorted_jittered_references


def test_frames_mode_equals_the_oracle_on_the_hosts_doubles_and_replays_in_a_graph():
    from dcase2019_task4_amd import metrics as M
    from dcase2019_task4_amd.inference import stitch_decode
    p, rec_win0, rec_frame0, L3s, T3, NC, _ = _stitch_inputs()
    total, n_rec = int(sum(L3s)), len(L3s)
    thr = torch.full((NC,), 0.5, device="cuda")
    win = torch.ones(NC, dtype=torch.int32, device="cuda")
    out = stitch_decode(p, rec_win0, rec_frame0, total, T3, thr, win, "uniform", want_timeline=False)
    assert int(out["err"].item()) == 0
    ev_ptr, ev_pairs = out["ev_ptr"].cpu().numpy(), out["ev_pairs"].cpu().numpy()
    est_cols = _decoded_cols(ev_ptr, ev_pairs, n_rec, NC)
    assert est_cols == ls.stitch_columns(ls.stitch_patterns(ls.stitch_lengths(rec_frame0[1].item() - 9), NC), NUM, DEN)
    assert max(len(c) for f in est_cols for c in f) > 200
    ref_cols = _sorted_refs(est_cols, 5)                             # (test_long_score_cpu: clusters within 64)
    ev, seg = se.set_counts(ref_cols, est_cols)
    ps = np.array(psds_np.set_counts(ref_cols, est_cols))
    ref = _ref_events(ref_cols)
    # the raw call on the table as the decoder left it: capacity, not the true count
    raw = ScoreCall((ev_ptr, out["ev_pairs"], NUM, DEN), ls.pack(ref_cols), n_rec, NC)
    assert raw.est_cap > ev_ptr[-1]
    _check_all(raw.run(), ev, seg, ps)
    # the Python route, eager ...
    c = M.long_event_counts(out, ref, 8, per_column=True)
    q = M.long_psds_counts(out, ref, 8, per_column=True)
    np.testing.assert_array_equal(c.ev_columns.cpu().numpy(), ev)
    np.testing.assert_array_equal(c.seg_columns.cpu().numpy(), seg)
    np.testing.assert_array_equal(q.columns.cpu().numpy(), ps)
    eager = (c.buf.cpu().numpy().copy(), q.buf.cpu().numpy().copy())
    np.testing.assert_array_equal(c.host()[0][0], ev.sum(0))
    # ... and ONE capture of stitch_decode + both scorers, replayed
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = stitch_decode(p, rec_win0, rec_frame0, total, T3, thr, win, "uniform", want_timeline=False)
        c_g = M.long_event_counts(out_g, ref, 8, per_column=True)
        q_g = M.long_psds_counts(out_g, ref, 8, per_column=True)
    for t in (out_g["ev_ptr"], out_g["ev_pairs"], c_g.ev_columns, c_g.seg_columns, q_g.columns):
        t.fill_(SENT)
    graph.replay()
    torch.cuda.synchronize()
    assert c_g.buf.cpu().numpy().tobytes() == eager[0].tobytes() and q_g.buf.cpu().numpy().tobytes() == eager[1].tobytes()
    np.testing.assert_array_equal(c_g.ev_columns.cpu().numpy(), ev)
    np.testing.assert_array_equal(q_g.columns.cpu().numpy(), ps)


def test_a_decoder_error_reaches_host_without_a_synchronisation_of_its_own():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd import metrics as M
    from dcase2019_task4_amd.inference import stitch_decode
    p, rec_win0, rec_frame0, L3s, T3, NC, _ = _stitch_inputs()
    total, n_rec = int(sum(L3s)), len(L3s)
    out = stitch_decode(p, rec_win0, rec_frame0, total, T3, 0.5, 1, "uniform", capacity=10, want_timeline=False)
    ref = _ref_events([[[] for _ in range(NC)] for _ in range(n_rec)])
    c = M.long_event_counts(out, ref, 8)
    with pytest.raises(_lib.SedError, match="decoded event table is invalid"):
        c.host()
    with pytest.raises(_lib.SedError, match="sed_long_psds_counts.*decoded event table"):
        M.long_psds_counts(out, ref, 8).host()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_validate_long_equals_the_oracle_on_get_long_predictions_at_two_points():
    from dcase2019_task4_amd import metrics as M
    from dcase2019_task4_amd.inference import LongRecordingSet, get_long_predictions
    labels = [f"c{i}" for i in range(10)]
    model, _ = gu.make_model(0)
    model.eval()
    rs = np.random.RandomState(21)
    feats = [(np.abs(rs.standard_normal((L, 64))) ** 2 * np.exp(rs.uniform(-6, 2, (L, 1))) + 1e-6).astype(np.float32)
             for L in (40, 64, 900)]
    names = ["a.wav", "b.wav", "c.wav"]
    lset = LongRecordingSet.from_arrays(feats, 64, scaler=_Scaler(64), filenames=names)
    _, timelines, _ = get_long_predictions(model, lset, labels, batch_size=8, return_posteriors=True)
    tl = torch.cat(timelines).cpu().numpy()
    points = [(np.median(tl, axis=0).astype(np.float32), [3, 1, 5, 3, 3, 7, 3, 1, 3, 5]), (float(np.quantile(tl, 0.6)), 1)]
    dfs = [get_long_predictions(model, lset, labels, batch_size=8, threshold=t, median_window=w) for t, w in points]
    cols = [se.columns_from_rows(df[["event_label", "onset", "offset", "filename"]].itertuples(index=False), names, labels)
            for df in dfs]
    assert all(len(df) > 5 for df in dfs)
    ref_cols = _sorted_refs(cols[0], 6)
    ref = M.RefEvents.from_dataframe(se.to_dataframe(ref_cols, names, labels), names, labels)
    psds = M.PSDSCounts(2, 10, "cuda")
    res = M.validate_long(model, lset, ref, [p[0] for p in points], [p[1] for p in points], batch_size=8, psds=psds)
    totals = psds.host()
    for k in range(2):
        ev, seg = se.set_counts(ref_cols, cols[k])
        ps = np.array(psds_np.set_counts(ref_cols, cols[k]))
        want_e, want_s = M.EventMetrics(labels, ev.sum(0)), M.SegmentMetrics(labels, seg.sum(0))
        assert res[k][0].class_wise == want_e.class_wise and res[k][1].class_wise == want_s.class_wise
        assert res[k][1].Ntn == want_s.Ntn
        np.testing.assert_array_equal(totals[k], ps.sum(0))
    d = lset.durations()
    np.testing.assert_array_equal(d, np.array([5, 8, 112]) * 8 / (44100 / 511))
    if (np.diff(ref.ptr_host).reshape(3, 10).sum(0) > 0).all():
        assert 0.0 <= M.PSDS.from_counts(totals, ref, d).psds() <= 1.0
    with pytest.raises(ValueError):
        M.validate_long(model, lset, ref, [0.5, 0.6], [1, 2, 3])
    with pytest.raises(ValueError):
        M.validate_long(model, lset, ref, [0.5], psds=psds)


# ---- error bits: each alone, nothing truncated -----------------------------------------------------------------------------------------
INSIDE = [(1.0 + k / 1024.0, 2.0) for k in range(65)]                 # 65 onsets inside one collar
ONE = [(1.01, 2.0)]


@pytest.mark.parametrize("ref,est,bit", [(INSIDE, ONE, 1), (ONE, INSIDE, 2), ([(2.0, 3.0), (1.0, 1.5)], ONE, 64),
                                         (ONE, [(2.0, 3.0), (1.0, 1.5)], 64), ([(1.0, 65536.5)], ONE, 4)])
def test_each_error_bit_alone(ref, est, bit):
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd import metrics as M
    ok_ref, ok_est = ls.spaced_column(np.random.RandomState(2), 30)
    ref_cols, est_cols = [[ok_ref, ref]], [[ok_est, est]]
    assert ls.expected_err(ref_cols, est_cols) == bit
    got = ScoreCall(ls.pack(est_cols), ls.pack(ref_cols), 1, 2).run(psds=False)
    assert got["err"] == bit
    assert tuple(got["ev"][0, 1]) == (0, len(ref), len(est)) and (got["seg"][0, 1] == 0).all()      # not scored, not truncated
    if bit != 4:                                                      # (the segment limit is the recording's)
        ev, seg = se.set_counts([[ok_ref]], [[ok_est]])
        np.testing.assert_array_equal(got["ev"][0, 0], ev[0, 0])
    ps = ScoreCall(ls.pack(est_cols), ls.pack(ref_cols), 1, 2).run(events=False)
    assert ps["err"] == (64 if bit == 64 else 0)                      # no matching and no segments in PSDS
    if bit != 64:
        np.testing.assert_array_equal(ps["ps"], np.array(psds_np.set_counts(ref_cols, est_cols)))
    with pytest.raises(_lib.SedError, match={1: "cluster of more than 64 reference", 2: "cluster of more than 64 estimated",
                                             4: "65 536 segments", 64: "onsets decrease"}[bit]):
        M.long_event_counts_from_events(_ref_events(est_cols), _ref_events(ref_cols)).host()


def test_the_limit_itself_is_scored():
    """64 onsets inside one collar on both sides: one cluster of 64 + 64, exact; 65 536 segments exactly."""
    ref, est = INSIDE[:64], [(on + 0.001, off) for on, off in INSIDE[:64]]
    ev, seg = se.set_counts([[ref]], [[est]])
    _check_all(ScoreCall(ls.pack([[est]]), ls.pack([[ref]]), 1, 1).run(psds=False), ev, seg, None, psds=False)
    assert ev[0, 0, 0] == 64
    ref, est = [(1.0, 65536.0)], [(65000.5, 65001.0)]
    ev, seg = se.set_counts([[ref]], [[est]])
    _check_all(ScoreCall(ls.pack([[est]]), ls.pack([[ref]]), 1, 1).run(psds=False), ev, seg, None, psds=False)
    assert seg[0, 0].sum() == 65536


@pytest.mark.parametrize("which", ["est", "ref"])
@pytest.mark.parametrize("ptr", [[0, 5, 3, 6], [0, 2, 4, 99], [-1, 2, 4, 6], [0, 2, 4, 1 << 40]])
def test_malformed_offsets_raise_bit_16_and_stay_inside_the_arrays(which, ptr):
    cols = [[[(float(2 * c + k), 2 * c + k + 0.5) for k in range(2)] for c in range(3)]]     # increasing across columns
    good = ls.pack(cols)
    bad = (np.array(ptr, np.int64), good[1], good[2])
    raw = ScoreCall(bad if which == "est" else good, bad if which == "ref" else good, 1, 3)
    got = raw.run()
    assert got["err"] == 16


def test_bad_host_arguments_return_before_any_launch():
    cols = [[[(0.0, 1.0)]]]
    raw = ScoreCall(ls.pack(cols), ls.pack(cols), 1, 1)
    raw.fill()
    l, p = raw.l, raw._lib.ptr
    head = list(raw._head())
    tail = [p(raw.ev_c), p(raw.seg_c), p(raw.ev_t), p(raw.seg_t), p(raw.err), p(raw.ws), raw.ws.numel(), raw._lib.stream_ptr()]
    assert l.sed_long_event_counts(*head, -0.1, 0.2, 1.0, *tail) == -1
    assert l.sed_long_event_counts(*head, 0.2, 0.2, 0.0, *tail) == -1
    assert l.sed_long_event_counts(*head[:12], 17, 0.2, 0.2, 1.0, *tail) == -1
    assert l.sed_long_event_counts(*head, 0.2, 0.2, 1.0, *tail[:6], 8, tail[7]) == -2
    assert l.sed_long_event_counts(None, *head[1:], 0.2, 0.2, 1.0, *tail) == -1
    assert l.sed_long_event_counts(head[0], None, 0.0, 0.0, None, None, *head[6:], 0.2, 0.2, 1.0, *tail) == -1
    assert l.sed_long_psds_counts(*head, 1.5, 0.5, 0.3, p(raw.ps_c), p(raw.ps_t), *tail[4:]) == -1
    got = raw.get()
    assert got["err"] == 0 and (got["ev"] == SENT).all() and (got["ps"] == SENT).all()                # nothing ran

"""-m gpu tests of the on-device validation scoring (dcase2019_task4_amd.metrics, csrc/score.hip) against the numpy / scipy
statement of the definitions in tests/sed_eval_np.py.

Every equality here is EXACT: the outputs are integers, and the seconds are the same fp64 operations on both sides
(``frame * pooling_time_ratio / (sample_rate / hop_length)``), so no tolerance is needed or allowed.  sed_eval itself is
absent from this image: parity with it is unpinned, agreement with the independent statement is what these tests pin."""
import numpy as np
import pandas as pd
import pytest
import torch

from oracle import features_np
from oracle import postprocess_np as pp
from oracle import synth
from tests import gpu_util as gu
from tests import sed_eval_np as se

pytestmark = pytest.mark.gpu
PTR, SR, HOP = 8, 44100, 511                    # pooling_time_ratio, config.py:17,19


def _names(N, NC):
    return [f"clip_{i}.wav" for i in range(N)], [f"c{i}" for i in range(NC)]


def _decoded(post, files, labels, thr=0.5, win=5):
    """cols[file][class] of the oracle's decode (the estimated events the device must form by itself)."""
    return se.columns_from_rows(pp.predictions(post, files, labels, PTR, SR, HOP, np.float32(thr), win), files, labels)


def _ref_events(ref_cols, files, labels):
    from dcase2019_task4_amd.metrics import RefEvents
    return RefEvents.from_dataframe(se.to_dataframe(ref_cols, files, labels), files, labels)


def _posteriors(N, T, NC):
    if T > 1024:          # slow posteriors for long clips: 16-frame steps, so that a column stays inside 64 events
        return torch.repeat_interleave(synth.make_posteriors(N + T, N, T // 16, NC), 16, dim=1)
    if T >= 40:
        return synth.make_posteriors(N + T, N, T, NC)
    return torch.tensor(np.random.RandomState(T).uniform(size=(N, T, NC)), dtype=torch.float32)


def _check_columns(counts, ref_cols, est_cols_per_point):
    ev, seg = counts.ev_columns.cpu().numpy(), counts.seg_columns.cpu().numpy()
    tot_ev, tot_seg = counts.host()
    for k, est_cols in enumerate(est_cols_per_point):
        want_ev, want_seg = se.set_counts(ref_cols, est_cols)
        np.testing.assert_array_equal(ev[k], want_ev)
        np.testing.assert_array_equal(seg[k], want_seg)
        np.testing.assert_array_equal(tot_ev[k], want_ev.sum(0))
        np.testing.assert_array_equal(tot_seg[k], want_seg.sum(0))


@pytest.mark.parametrize("T", [78, 108])
def test_event_counts_vs_helper_where_first_fit_loses_matches(T):
    """64 clips x 10 classes of structured posteriors against references made from the window-7 decode of the same posteriors
    (events dropped, moved by up to 0.3 s at both ends, some duplicated 0.1 s later: overlapping references).  The test first
    asserts two facts about its own inputs - a maximum matching finds more pairs than first-fit does, and no column exceeds
    the 64-event limit - so that a changed generator cannot quietly make it vacuous."""
    from dcase2019_task4_amd.metrics import event_counts
    N, NC = 64, 10
    files, labels = _names(N, NC)
    post = synth.make_posteriors(1, N, T)
    est = _decoded(post.numpy(), files, labels)
    ref = se.jittered_references(_decoded(post.numpy(), files, labels, win=7), np.random.RandomState(7))
    pairs = [(r, e) for rf, ef in zip(ref, est) for r, e in zip(rf, ef)]
    optimal, first_fit = sum(se.optimal_ntp(r, e) for r, e in pairs), sum(se.first_fit_ntp(r, e) for r, e in pairs)
    per_column = max(max(len(r), len(e)) for r, e in pairs)
    print(f"T {T}: {sum(len(e) for _, e in pairs)} estimated, {sum(len(r) for r, _ in pairs)} reference events, optimal Ntp "
          f"{optimal}, first-fit {first_fit}, at most {per_column} events in a column")
    assert optimal > first_fit and per_column <= 64
    counts = event_counts(post.cuda(), _ref_events(ref, files, labels), pooling_time_ratio=PTR, per_column=True)
    _check_columns(counts, ref, [est])
    assert int(counts.host()[0][0, :, 0].sum()) == optimal


@pytest.mark.parametrize("N,T,NC,win", [(1, 1, 3, 5), (2, 5, 2, 9), (4, 200, 16, 4), (257, 78, 10, 5),
                                        (3, 2048, 16, 5)])
def test_event_counts_vs_helper_odd_shapes(N, T, NC, win):
    """The odd shapes of test_postprocess_kernel_vs_oracle: one-frame clips, columns shorter than the window, an even window,
    16 classes (a 1024-thread workgroup), more clips than any single-clip loop would see - and the largest supported shape
    (2048 frames x 16 classes: 82 KB of LDS per workgroup, 190 one-second segments per file)."""
    from dcase2019_task4_amd.metrics import event_counts
    files, labels = _names(N, NC)
    post = _posteriors(N, T, NC)
    est = _decoded(post.numpy(), files, labels, win=win)
    ref = se.jittered_references(_decoded(post.numpy(), files, labels, win=7), np.random.RandomState(N + T))
    # make_posteriors' alternating column decodes to T / 2 one-frame events at an odd window: 100 at T = 200.  A column holds
    # at most 64 (the over-limit error has its own test), so the references of such a column stop at the 64th.
    ref = [[col[:64] for col in file_cols] for file_cols in ref]
    assert max(len(col) for file_cols in est for col in file_cols) <= 64
    counts = event_counts(post.cuda(), _ref_events(ref, files, labels), (0.5,), (win,), PTR, per_column=True)
    _check_columns(counts, ref, [est])


def test_given_events_dense_overlapping_columns_need_augmenting_paths():
    """The matching stage alone (events given, as the DataFrame route uses it): random heavily overlapping lists of up to 64
    events per column and side.  Asserted about the inputs first: first-fit in the order the device holds the events
    (sorted by onset), from either side, finds fewer pairs than a maximum matching."""
    from dcase2019_task4_amd.metrics import event_counts_from_events
    N, NC = 24, 10
    files, labels = _names(N, NC)
    rs = np.random.RandomState(11)
    ref, est = se.dense_events(rs, N, NC, 64), se.dense_events(rs, N, NC, 64)
    ref[0][0] = [(1.0, 2.0), (1.05, 2.4)]                       # the sorted hand case of tests/test_metrics_cpu.py
    est[0][0] = [(0.9, 2.15), (1.0, 1.9)]
    ref[1][0], est[1][0] = [(0.5, 2.0)], [(0.0, 2.0)]           # |d onset| == t_collar exactly in the second call below
    assert se.optimal_ntp(ref[1][0], est[1][0], t_collar=0.5) == 1 and se.optimal_ntp(ref[1][0], est[1][0]) == 0
    pairs = [(r, e) for rf, ef in zip(ref, est) for r, e in zip(rf, ef)]
    optimal = sum(se.optimal_ntp(r, e) for r, e in pairs)
    assert optimal > sum(se.first_fit_ntp(r, e) for r, e in pairs)
    assert optimal > sum(se.first_fit_ntp(r, e, est_major=True) for r, e in pairs)
    assert max(max(len(r), len(e)) for r, e in pairs) == 64
    counts = event_counts_from_events(_ref_events(est, files, labels), _ref_events(ref, files, labels), per_column=True)
    _check_columns(counts, ref, [est])
    # other collars and a finer segment grid
    counts = event_counts_from_events(_ref_events(est, files, labels), _ref_events(ref, files, labels), t_collar=0.5,
                                      percentage_of_length=0.5, time_resolution=0.25, per_column=True)
    want_ev, want_seg = se.set_counts(ref, est, t_collar=0.5, percentage_of_length=0.5, res=0.25)
    np.testing.assert_array_equal(counts.ev_columns.cpu().numpy()[0], want_ev)
    np.testing.assert_array_equal(counts.seg_columns.cpu().numpy()[0], want_seg)


def test_sweep_of_operating_points_in_one_launch():
    """K = 12 (threshold, window) points in one launch == 12 single-point launches == the helper; totals == column sums;
    two runs bit-identical."""
    from dcase2019_task4_amd.metrics import event_counts
    N, T, NC = 64, 78, 10
    files, labels = _names(N, NC)
    post = synth.make_posteriors(1, N, T)
    ref_cols = se.jittered_references(_decoded(post.numpy(), files, labels, win=7), np.random.RandomState(7))
    ref = _ref_events(ref_cols, files, labels)
    points = [(t, w) for t in (0.1, 0.3, 0.5, 0.7, 0.9) for w in (1, 5, 9)][:12]
    thr, win = [p[0] for p in points], [p[1] for p in points]
    dev = post.cuda()
    sweep = event_counts(dev, ref, thr, win, PTR, per_column=True)
    _check_columns(sweep, ref_cols, [_decoded(post.numpy(), files, labels, t, w) for t, w in points])
    again = event_counts(dev, ref, thr, win, PTR, per_column=True)
    assert torch.equal(sweep.buf, again.buf)
    assert torch.equal(sweep.ev_columns, again.ev_columns) and torch.equal(sweep.seg_columns, again.seg_columns)
    assert torch.equal(sweep.ev, sweep.ev_columns.sum(1, dtype=torch.int64))
    assert torch.equal(sweep.seg, sweep.seg_columns.sum(1, dtype=torch.int64))
    for k, (t, w) in enumerate(points):
        one = event_counts(dev, ref, (t,), (w,), PTR, per_column=True)
        assert torch.equal(one.ev_columns[0], sweep.ev_columns[k]) and torch.equal(one.seg_columns[0], sweep.seg_columns[k])
        assert torch.equal(one.ev[0], sweep.ev[k]) and torch.equal(one.seg[0], sweep.seg[k])
    # batches chained into one set of totals == the whole set at once
    chained = None
    for i0 in range(0, N, 24):
        chained = event_counts(dev[i0:i0 + 24], ref, thr, win, PTR, clip_offset=i0, counts=chained)
    assert torch.equal(chained.buf, sweep.buf)


def test_a_column_over_the_limit_raises_and_the_limit_itself_is_scored():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.metrics import event_counts, event_counts_from_events
    files, labels = _names(2, 3)

    def cols(n):
        c = [[[] for _ in labels] for _ in files]
        c[1][2] = [(0.5 * i, 0.5 * i + 0.25) for i in range(n)]
        return c
    full = _ref_events(cols(64), files, labels)
    ev, seg = event_counts_from_events(full, full).host()                    # 64 events on both sides: every mask bit used
    assert ev[0].tolist() == [[0, 0, 0], [0, 0, 0], [64, 64, 64]]
    assert seg[0].tolist() == [[0, 0, 0, 32], [0, 0, 0, 32], [32, 0, 0, 0]]
    over = _ref_events(cols(65), files, labels)
    assert over.max_per_column == 65
    with pytest.raises(_lib.SedError, match="more than 64 reference events"):
        event_counts_from_events(full, over).host()
    with pytest.raises(_lib.SedError, match="more than 64 estimated events"):
        event_counts_from_events(over, full).check()
    with pytest.raises(_lib.SedError, match="more than 64 reference events"):
        event_counts(synth.make_posteriors(3, 2, 78, 3).cuda(), over, pooling_time_ratio=PTR).host()
    # decoded events over the limit: an alternating column of 200 frames holds 100 one-frame events at window 1
    post = torch.full((2, 200, 3), 0.1)
    post[0, ::2, 1] = 0.9
    with pytest.raises(_lib.SedError, match="more than 64 estimated events"):
        event_counts(post.cuda(), full, (0.5,), (1,), PTR).host()


class _DS:
    def __init__(self, x):
        self.x = x
        self.filenames = pd.Series([f"clip_{i}.wav" for i in range(len(x))])

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], torch.zeros(1)


class _EvalDS(_DS):
    """DataLoadDf-like: get_sample -> (linear mel, label)."""

    def get_sample(self, i):
        return self.x[i], np.zeros(1)


class _Enc:
    def __init__(self, labels):
        self.labels = labels

    def decode_strong(self, m):
        return pp.decode_strong(m, self.labels)


def test_dataframe_route_and_fused_route_agree_on_a_real_model():
    """compute_strong_metrics(get_predictions(...), valid_df) and validate(...) on an eval-mode CRNN, 37 clips in batches of
    16 (ragged last batch), through a per-clip dataset and a ResidentFeatureSet.for_eval: same counts, and the number
    main.py:348 reads equals the helper's."""
    from dcase2019_task4_amd.features import LogMelTransform, Scaler
    from dcase2019_task4_amd.inference import eval_batches, get_predictions
    from dcase2019_task4_amd.metrics import RefEvents, compute_strong_metrics, validate
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    N, T = 37, 628
    rs = np.random.RandomState(4)
    feats = []
    for k in range(N):
        L = (628, 500, 700, 640)[k % 4]
        gain = np.repeat(rs.choice([0.02, 1.0, 30.0], size=(L + 39) // 40), 40)[:L]        # level steps: posteriors that move
        feats.append((np.abs(rs.standard_normal((L, 64))) * 3.0 * gain[:, None]).astype(np.float32))
    sc = Scaler()
    sc.calculate_scaler([features_np.transform_chain(f, T) for f in feats[:4]])
    tr = LogMelTransform(T, sc)
    per_clip = _DS([tr(torch.tensor(f)[None])[0].cpu() for f in feats])
    resident = ResidentFeatureSet.for_eval(_EvalDS(feats), T, sc)
    model, _ = gu.make_model(0)
    model.eval()
    files, labels = per_clip.filenames.tolist(), [f"c{i}" for i in range(10)]
    def posteriors(ds):
        with torch.no_grad():
            return torch.cat([model(x)[0] for _, _, x in eval_batches(ds, 16, "cuda")]).cpu().numpy()
    ref_cols = se.jittered_references(_decoded(posteriors(per_clip), files, labels, win=7), np.random.RandomState(3))
    valid_df = se.to_dataframe(ref_cols, files, labels)
    ref = RefEvents.from_dataframe(valid_df, files, labels)
    for ds in (per_clip, resident):
        est = _decoded(posteriors(ds), files, labels)
        assert sum(len(c) for f in est for c in f) > 20
        want_ev, want_seg = (c.sum(0) for c in se.set_counts(ref_cols, est))
        want_f = se.class_wise_average_f(want_ev)
        [(ev_m, seg_m)] = validate(model, ds, ref, PTR, batch_size=16)
        df_m = compute_strong_metrics(get_predictions(model, ds, _Enc(labels).decode_strong, PTR, batch_size=16), valid_df)
        # the DataFrame route knows the classes of its two tables only (evaluation_measures.py:136-139): a class in neither
        # has no counts there - and, with Nref == 0, no part in the class-wise average on either route
        assert set(df_m.event_label_list) == {l for l, c in zip(labels, want_ev) if c[1] or c[2]} != set()
        nothing = {"Ntp": 0, "Nref": 0, "Nsys": 0}
        for m in (ev_m, df_m):
            got = np.array([[c["Ntp"], c["Nref"], c["Nsys"]] for c in (m.class_wise.get(l, nothing) for l in labels)])
            np.testing.assert_array_equal(got, want_ev)
            assert m.results_class_wise_average_metrics()["f_measure"]["f_measure"] == want_f
        np.testing.assert_array_equal(np.array([[c["Ntp"], c["Nfp"], c["Nfn"]] for c in (seg_m.class_wise[l] for l in labels)]),
                                      want_seg[:, :3])
        assert [seg_m.Ntn[l] for l in labels] == want_seg[:, 3].tolist()
        assert model.training is False
    # refusals, like get_predictions
    from dcase2019_task4_amd import _lib
    with pytest.raises(_lib.SedError):
        validate(torch.nn.Linear(2, 2).cuda(), per_clip, ref, PTR)
    with pytest.raises(ValueError):
        validate(model, _DS(per_clip.x[:5]), ref, PTR)


def _reference_weak_f(pred_weak, labels, thresholds_):
    """evaluation_measures.py:59-81 restated: binarise, intermediate_at_measures, the masked F."""
    thresh = 0.5 if thresholds_ is None else np.asarray(thresholds_, np.float32)
    est = (pred_weak > thresh).astype(int)
    tp = (est + labels == 2).sum(axis=0).astype(float)
    fp = (est - labels == 1).sum(axis=0).astype(float)
    fn = (labels - est == 1).sum(axis=0).astype(float)
    tn = (est + labels == 0).sum(axis=0).astype(float)
    f = np.zeros(labels.shape[1])
    mask = 2 * tp + fp + fn != 0
    f[mask] = 2 * tp[mask] / (2 * tp + fp + fn)[mask]
    return f, np.stack([tp, fp, fn, tn], 1)


def test_get_f_measure_by_class_and_weak_counts():
    from dcase2019_task4_amd.metrics import get_f_measure_by_class, weak_counts
    N, NC = 150, 10
    rs = np.random.RandomState(21)
    weak = torch.tensor(rs.uniform(size=(N, NC)), dtype=torch.float32)
    weak[:, 3] = 0.2                                    # never predicted: tp + fp == 0
    y2 = torch.tensor((rs.uniform(size=(N, NC)) < 0.3).astype(np.float32))
    y2[:, 7] = 0                                        # no positives and ...
    weak[:, 7] = 0.1                                    # ... no predictions: 2 tp + fp + fn == 0 -> F = 0 by the mask
    y3 = torch.tensor(rs.uniform(size=(N, 12, NC)).astype(np.float32)) * y2[:, None, :]
    y3[:, 5, :] = torch.maximum(y3[:, 5, :], y2 * 0.9)  # max over time > 0.5 exactly where y2 is set

    class Fixed(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.dummy = torch.nn.Parameter(torch.zeros(1))
            self.pos = 0

        def forward(self, inp):
            out = weak[self.pos:self.pos + inp.shape[0]].cuda()
            self.pos += inp.shape[0]
            return out[:, None, :].expand(-1, 4, -1), out

    def loader(y, bs=64):
        return [(torch.zeros(len(y[i:i + bs]), 1, 8, 8), y[i:i + bs]) for i in range(0, N, bs)]
    per_class = [float(v) for v in rs.uniform(0.2, 0.8, size=NC)]
    for thresholds_ in (None, per_class):
        want_f, want_counts = _reference_weak_f(weak.numpy(), y2.numpy().astype(int), thresholds_)
        for y in (y2, y3):
            got = get_f_measure_by_class(Fixed().cuda(), NC, loader(y), thresholds_)
            np.testing.assert_array_equal(got, want_f)
        thr = [0.5] * NC if thresholds_ is None else thresholds_
        np.testing.assert_array_equal(weak_counts(weak.cuda(), y2.cuda(), thr).cpu().numpy()[0], want_counts)
    assert want_f[7] == 0.0 and want_f[3] == 0.0
    # K threshold sets in one launch
    sets = np.stack([np.full(NC, 0.5, np.float32), np.asarray(per_class, np.float32)])
    got = weak_counts(weak.cuda(), y2.cuda(), sets).cpu().numpy()
    np.testing.assert_array_equal(got[0], _reference_weak_f(weak.numpy(), y2.numpy().astype(int), None)[1])
    np.testing.assert_array_equal(got[1], want_counts)


def test_event_counts_in_a_captured_graph():
    from dcase2019_task4_amd.metrics import Counts, event_counts, operating_points
    N, T, NC = 24, 78, 10
    files, labels = _names(N, NC)
    post = synth.make_posteriors(2, N, T)
    ref_cols = se.jittered_references(_decoded(post.numpy(), files, labels, win=7), np.random.RandomState(5))
    ref = _ref_events(ref_cols, files, labels)
    dev = post.cuda()
    thr, win = operating_points((0.4, 0.5), (5, 7), "cuda")
    eager = event_counts(dev, ref, thr, win, PTR)
    counts = Counts(2, NC, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        event_counts(dev, ref, thr, win, PTR, counts=counts)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        event_counts(dev, ref, thr, win, PTR, counts=counts)
    for _ in range(2):
        counts.buf.zero_()
        graph.replay()
        assert torch.equal(counts.buf, eager.buf)
    np.testing.assert_array_equal(counts.host()[0][1], se.set_counts(ref_cols, _decoded(post.numpy(), files, labels, 0.5, 7))[0].sum(0))

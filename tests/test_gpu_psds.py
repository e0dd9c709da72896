"""-m gpu tests of the on-device PSDS intersection counts (dcase2019_task4_amd.metrics.psds_counts, csrc/score.hip
k_psds_counts) against the plain-loop statement of the definitions in tests/psds_np.py.

Every equality here is EXACT: the outputs are integers, the seconds are the same fp64 operations on both sides, and every
criterion is the same sequential fp64 sum, one division and one comparison on both sides, so no tolerance is needed or
allowed.  psds_eval itself is absent from this image: parity with it is unpinned, agreement with the independent statement
is what these tests pin."""
import numpy as np
import pandas as pd
import pytest
import torch

from oracle import postprocess_np as pp
from oracle import synth
from tests import gpu_util as gu
from tests import psds_np as ps
from tests import sed_eval_np as se

pytestmark = pytest.mark.gpu
PTR, SR, HOP = 8, 44100, 511                    # pooling_time_ratio, config.py:17,19
EPS = 2.0 ** -52


def _names(N, NC):
    return [f"clip_{i}.wav" for i in range(N)], [f"c{i}" for i in range(NC)]


def _decoded(post, files, labels, thr=0.5, win=5):
    """cols[file][class] of the oracle's decode (the detections the device must form by itself)."""
    return se.columns_from_rows(pp.predictions(post, files, labels, PTR, SR, HOP, np.float32(thr), win), files, labels)


def _ref_events(cols, files, labels):
    from dcase2019_task4_amd.metrics import RefEvents
    return RefEvents.from_dataframe(se.to_dataframe(cols, files, labels), files, labels)


def _posteriors(N, T, NC):
    if T > 1024:          # slow posteriors for long clips: 16-frame steps, so that a column stays inside 64 events
        return torch.repeat_interleave(synth.make_posteriors(N + T, N, T // 16, NC), 16, dim=1)
    if T >= 40:
        return synth.make_posteriors(N + T, N, T, NC)
    return torch.tensor(np.random.RandomState(T).uniform(size=(N, T, NC)), dtype=torch.float32)


def _check(counts, ref_cols, est_cols_per_point, **criteria):
    """Per-column and total counts of every operating point equal the helper's; returns the helper's [K, N, NC, 2 + NC]."""
    got, total = counts.columns.cpu().numpy(), counts.host()
    want = np.array([ps.set_counts(ref_cols, est_cols, **criteria) for est_cols in est_cols_per_point], np.int64)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(total, want.sum(1))
    return want


def test_structured_posteriors_at_five_thresholds():
    """32 clips x 10 classes of structured posteriors against jittered references of the window-7 decode, K = 5 thresholds at
    window 5.  Asserted about the inputs first, with the helper, so that a changed generator cannot make the test vacuous: a
    detection fails DTC, a cross-trigger is counted, a ground truth overlaps a relevant detection and still fails GTC, a
    column holds two overlapping references of one class, and no column exceeds the 64-event limit."""
    from dcase2019_task4_amd.metrics import psds_counts
    N, T, NC = 32, 78, 10
    files, labels = _names(N, NC)
    post = synth.make_posteriors(1, N, T, NC)
    thresholds = (0.1, 0.3, 0.5, 0.7, 0.9)
    est = [_decoded(post.numpy(), files, labels, t, 5) for t in thresholds]
    ref = se.jittered_references(_decoded(post.numpy(), files, labels, win=7), np.random.RandomState(7))
    counts = psds_counts(post.cuda(), _ref_events(ref, files, labels), thresholds, (5,), PTR, per_column=True)
    want = _check(counts, ref, est)
    gtc_misses = 0
    for est_cols in est:
        for ref_file, est_file in zip(ref, est_cols):
            for r, e in zip(ref_file, est_file):
                r = sorted(r)
                relevant = ps.relevant_mask(e, r, 0.5)
                found = ps.found_mask(e, r, relevant, 0.5)
                gtc_misses += sum(1 for g, f in zip(r, found)
                                  if not f and any(rel and ps.intersection(d, g) > 0 for d, rel in zip(e, relevant)))
    overlapping = sum(1 for f in ref for col in f if any(ps.intersection(a, b) > 0 for i, a in enumerate(col) for b in col[i + 1:]))
    per_column = max(max(len(r), len(e)) for est_cols in est for rf, ef in zip(ref, est_cols) for r, e in zip(rf, ef))
    print(f"TP {want[..., 0].sum()}, FP (DTC failures) {want[..., 1].sum()}, cross-triggers {want[..., 2:].sum()}, ground truths "
          f"overlapping a relevant detection that fail GTC {gtc_misses}, columns with overlapping references {overlapping}, "
          f"at most {per_column} events in a column")
    assert want[..., 1].sum() > 0 and want[..., 2:].sum() > 0 and gtc_misses > 0 and overlapping > 0 and per_column <= 64
    assert want[..., 0].sum() > 0
    for c in range(NC):
        assert not want[:, :, c, 2 + c].any()                       # CT[c][c] is 0


@pytest.mark.parametrize("N,T,NC,win", [(1, 1, 3, 5), (2, 5, 2, 9), (4, 200, 16, 4), (257, 78, 10, 5), (3, 2048, 16, 5),
                                        (2, 40, 1, 5)])
def test_psds_counts_vs_helper_odd_shapes(N, T, NC, win):
    """The odd shapes of test_event_counts_vs_helper_odd_shapes - one-frame clips, columns shorter than the window, an even
    window, 16 classes (a 1024-thread workgroup), many clips, the largest supported shape (2048 frames x 16 classes: 97 KB of
    LDS per workgroup) - and a single class: no cross-trigger partner."""
    from dcase2019_task4_amd.metrics import psds_counts
    files, labels = _names(N, NC)
    post = _posteriors(N, T, NC)
    est = _decoded(post.numpy(), files, labels, win=win)
    ref = se.jittered_references(_decoded(post.numpy(), files, labels, win=7), np.random.RandomState(N + T))
    # an alternating column decodes to T / 2 one-frame events at an odd window; a column holds at most 64 (the over-limit
    # error has its own test), so the references of such a column stop at the 64th
    ref = [[col[:64] for col in file_cols] for file_cols in ref]
    assert max(len(col) for file_cols in est for col in file_cols) <= 64
    counts = psds_counts(post.cuda(), _ref_events(ref, files, labels), (0.5,), (win,), PTR, per_column=True)
    want = _check(counts, ref, [est])
    assert want.shape == (1, N, NC, 2 + NC)


def _hand_files(NC=10):
    """Three files of dyadic hand columns that sit exactly on each threshold.
    file 0: class 0 - detection (1, 2) against ground truth (1.5, 3): ratio exactly 0.5, relevant at dtc 0.5 and not one ulp
            above; the ground truth is covered by 0.5 of 1.5 s only.  class 1 - the same detection against (1.5, 2.5): the
            ground truth is covered by exactly 0.5 of its 1 s.
    file 1: class 3 holds a detection (0, 1) and no ground truth, class 4 a ground truth (0, 0.3): the intersection is the
            double 0.3 itself, 0.3 / 1 >= 0.3 - a cross-trigger at cttc 0.3 and not one ulp above.
    file 2: class 5 - a zero-length detection and a zero-length ground truth beside a matching pair."""
    ref = [[[] for _ in range(NC)] for _ in range(3)]
    est = [[[] for _ in range(NC)] for _ in range(3)]
    est[0][0], ref[0][0] = [(1.0, 2.0)], [(1.5, 3.0)]
    est[0][1], ref[0][1] = [(1.0, 2.0)], [(1.5, 2.5)]
    est[1][3], ref[1][4] = [(0.0, 1.0)], [(0.0, 0.3)]
    est[2][5], ref[2][5] = [(2.0, 2.0), (2.0, 3.0)], [(2.0, 2.0), (2.0, 3.0)]
    return ref, est


def test_hand_columns_exactly_on_each_threshold():
    from dcase2019_task4_amd.metrics import psds_counts_from_events
    NC = 10
    files, labels = _names(3, NC)
    ref, est = _hand_files(NC)
    dev_ref, dev_est = _ref_events(ref, files, labels), _ref_events(est, files, labels)
    at = _check(psds_counts_from_events(dev_est, dev_ref, per_column=True), ref, [est])[0]
    above = dict(dtc=0.5 + EPS, gtc=0.5 + EPS, cttc=float(np.nextafter(0.3, 1.0)))
    over = _check(psds_counts_from_events(dev_est, dev_ref, per_column=True, **above), ref, [est], **above)[0]
    # (TP, FP) of file 0: DTC tie in class 0 (and 0.5 of 1.5 s is no true positive), GTC tie in class 1
    assert at[0, 0, :2].tolist() == [0, 0] and over[0, 0, :2].tolist() == [0, 1]
    assert at[0, 1, :2].tolist() == [1, 0] and over[0, 1, :2].tolist() == [0, 1]
    # file 1: the detection of class 3 is a false positive and, at the tie, a cross-trigger of class 4 alone
    assert at[1, 3, 1] == 1 and at[1, 3, 2:].tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0, 0] and not over[1, 3, 2:].any()
    # file 2: the zero-length detection is a false positive, the zero-length ground truth is never found
    assert at[2, 5, :2].tolist() == [1, 1]
    zero = dict(dtc=0.0, gtc=0.0, cttc=0.0)
    at_zero = _check(psds_counts_from_events(dev_est, dev_ref, per_column=True, **zero), ref, [est], **zero)[0]
    assert at_zero[2, 5, :2].tolist() == [1, 1] and at_zero[1, 3, :2].tolist() == [0, 0]      # no ground truth: 0 / 1 >= 0


def test_given_events_dense_columns_and_three_sets_of_criteria():
    """The criteria alone (events given): random heavily overlapping lists of up to 64 events per column and side in 24 files,
    plus the three hand files, at the task's criteria, at (0.1, 0.9, 0.05) and with all three at 0."""
    from dcase2019_task4_amd.metrics import psds_counts_from_events
    N, NC = 24, 10
    files, labels = _names(N + 3, NC)
    rs = np.random.RandomState(11)
    hand_ref, hand_est = _hand_files(NC)
    ref, est = se.dense_events(rs, N, NC, 64) + hand_ref, se.dense_events(rs, N, NC, 64) + hand_est
    assert max(max(len(r), len(e)) for rf, ef in zip(ref, est) for r, e in zip(rf, ef)) == 64
    dev_ref, dev_est = _ref_events(ref, files, labels), _ref_events(est, files, labels)
    for criteria in (dict(), dict(dtc=0.1, gtc=0.9, cttc=0.05), dict(dtc=0.0, gtc=0.0, cttc=0.0)):
        want = _check(psds_counts_from_events(dev_est, dev_ref, per_column=True, **criteria), ref, [est], **criteria)
        print(criteria, "TP", want[..., 0].sum(), "FP", want[..., 1].sum(), "CT", want[..., 2:].sum())
        assert want[..., 0].sum() > 0
    # at 0 every detection of positive length is relevant: the zero-length one is the only false positive, and no cross-trigger
    assert want[..., 1].sum() == 1 and want[..., 2:].sum() == 0


def test_batches_accumulate_and_a_sweep_equals_single_points():
    """Clips 0 .. 15 and 16 .. 31 with clip_offset into one PSDSCounts == one call over 32; K = 50 thresholds in one launch ==
    50 launches of one."""
    from dcase2019_task4_amd.metrics import psds_counts
    N, T, NC = 32, 78, 10
    files, labels = _names(N, NC)
    post = synth.make_posteriors(1, N, T, NC)
    ref = _ref_events(se.jittered_references(_decoded(post.numpy(), files, labels, win=7), np.random.RandomState(7)), files, labels)
    dev = post.cuda()
    thr = [float(v) for v in np.linspace(0.01, 0.99, 50)]
    whole = psds_counts(dev, ref, thr, (5,), PTR, per_column=True)
    assert whole.totals.shape == (50, NC, 2 + NC) and int(whole.totals.sum()) > 0
    assert torch.equal(whole.totals, whole.columns.sum(1, dtype=torch.int64))
    halves = psds_counts(dev[:16], ref, thr, (5,), PTR)
    assert psds_counts(dev[16:], ref, thr, (5,), PTR, clip_offset=16, counts=halves) is halves
    assert torch.equal(halves.buf, whole.buf)
    for k, t in enumerate(thr):
        one = psds_counts(dev, ref, (t,), (5,), PTR, per_column=True)
        assert torch.equal(one.totals[0], whole.totals[k]) and torch.equal(one.columns[0], whole.columns[k])
    whole.host()
    with pytest.raises(ValueError):
        psds_counts(dev, ref, thr, (5,), PTR, dtc=0.7, counts=whole)            # totals of other criteria


def test_a_column_over_the_limit_raises_and_the_limit_itself_is_scored():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.metrics import psds_counts, psds_counts_from_events
    files, labels = _names(2, 3)

    def cols(n):
        c = [[[] for _ in labels] for _ in files]
        c[1][2] = [(0.5 * i, 0.5 * i + 0.25) for i in range(n)]
        return c
    full = _ref_events(cols(64), files, labels)
    totals = psds_counts_from_events(full, full).host()                      # 64 events on both sides: every lane used
    assert totals[0].tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [64, 0, 0, 0, 0]]
    over = _ref_events(cols(65), files, labels)
    with pytest.raises(_lib.SedError, match="more than 64 reference events"):
        psds_counts_from_events(full, over).host()
    with pytest.raises(_lib.SedError, match="more than 64 estimated events"):
        psds_counts_from_events(over, full).check()
    with pytest.raises(_lib.SedError, match="more than 64 reference events"):
        psds_counts(synth.make_posteriors(3, 2, 78, 3).cuda(), over, pooling_time_ratio=PTR).host()
    # decoded detections over the limit: an alternating column of 200 frames holds 100 one-frame events at window 1
    post = torch.full((2, 200, 3), 0.1)
    post[0, ::2, 1] = 0.9
    with pytest.raises(_lib.SedError, match="more than 64 estimated events"):
        psds_counts(post.cuda(), full, (0.5,), (1,), PTR).host()
    # a window of 0: refused on the host, and by the kernel's error word when the operating points are device tensors
    with pytest.raises(_lib.SedError):
        psds_counts(post.cuda(), full, (0.5,), (0,), PTR)
    thr, win = torch.tensor([0.5], device="cuda"), torch.tensor([0], dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.SedError, match="median window"):
        psds_counts(post[:, :40].cuda(), full, thr, win, PTR).host()


class _DS:
    def __init__(self, x):
        self.x = x
        self.filenames = pd.Series([f"clip_{i}.wav" for i in range(len(x))])

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], torch.zeros(1)


def test_validate_fills_the_psds_counts_from_the_same_forward():
    """A hot-path CRNN at the smallest legal shape (64 input frames, batches of 4, 10 classes, random parameters) over 10 clips
    (ragged last batch): the totals validate() leaves in the PSDSCounts equal psds_counts applied to the model's eval-mode
    strong output batch by batch, and equal the helper's; the returned F-measure pairs equal those of a call without psds."""
    from dcase2019_task4_amd.inference import eval_batches
    from dcase2019_task4_amd.metrics import PSDS, PSDSCounts, psds_counts, validate
    N, T, B, NC = 10, 64, 4, 10
    rs = np.random.RandomState(8)
    gain = np.repeat(rs.choice([0.05, 1.0, 20.0], size=(N, 1, T // 8, 1)), 8, axis=2)       # level steps: posteriors that move
    ds = _DS(list(synth.make_input(5, N, T) * torch.tensor(gain, dtype=torch.float32)))
    model, _ = gu.make_model(0)
    model.eval()
    files, labels = ds.filenames.tolist(), [f"c{i}" for i in range(NC)]
    with torch.no_grad():
        strong = torch.cat([model(x)[0] for _, _, x in eval_batches(ds, B, "cuda")])
    post = strong.cpu().numpy()
    assert post.shape == (N, T // 8, NC)
    thresholds = [float(v) for v in np.quantile(post, (0.3, 0.5, 0.7))]                      # operating points with detections
    ref_cols = se.jittered_references(_decoded(post, files, labels, thresholds[1], 3), np.random.RandomState(3), p_drop=0.3)
    ref = _ref_events(ref_cols, files, labels)
    criteria = dict(dtc=0.6, gtc=0.4, cttc=0.2)
    psds = PSDSCounts(3, NC, "cuda", **criteria)
    with_psds = validate(model, ds, ref, PTR, thresholds, (3,), batch_size=B, psds=psds)
    without = validate(model, ds, ref, PTR, thresholds, (3,), batch_size=B)
    direct = None
    for i0 in range(0, N, B):
        direct = psds_counts(strong[i0:i0 + B], ref, thresholds, (3,), PTR, clip_offset=i0, counts=direct, **criteria)
    assert torch.equal(psds.buf, direct.buf)
    want = np.array([ps.set_counts(ref_cols, _decoded(post, files, labels, t, 3), **criteria) for t in thresholds]).sum(1)
    np.testing.assert_array_equal(psds.host(), want)
    print("TP", want[..., 0].sum(), "FP", want[..., 1].sum(), "CT", want[..., 2:].sum())
    assert want[..., :2].sum() > 0
    assert len(with_psds) == len(without) == 3
    for (ev_a, seg_a), (ev_b, seg_b) in zip(with_psds, without):
        assert ev_a.class_wise == ev_b.class_wise and seg_a.class_wise == seg_b.class_wise and seg_a.Ntn == seg_b.Ntn
        assert str(ev_a) == str(ev_b) and str(seg_a) == str(seg_b)
    assert model.training is False
    with pytest.raises(ValueError):
        validate(model, ds, ref, PTR, thresholds[:2], (3,), batch_size=B, psds=psds)         # counts of another K
    if all(n > 0 for n in np.diff(ref.ptr_host).reshape(N, NC).sum(0)):
        score = PSDS.from_counts(psds, ref, 10.0).psds()
        assert 0.0 <= score <= 1.0


def test_the_same_call_twice_is_bit_identical_and_the_launch_is_capturable():
    from dcase2019_task4_amd.metrics import PSDSCounts, operating_points, psds_counts
    N, T, NC = 24, 78, 10
    files, labels = _names(N, NC)
    post = synth.make_posteriors(2, N, T, NC)
    ref = _ref_events(se.jittered_references(_decoded(post.numpy(), files, labels, win=7), np.random.RandomState(5)), files, labels)
    dev = post.cuda()
    thr, win = operating_points((0.4, 0.5, 0.6), (5, 7, 3), "cuda")
    first = psds_counts(dev, ref, thr, win, PTR, per_column=True)
    again = psds_counts(dev, ref, thr, win, PTR, per_column=True)
    assert torch.equal(first.buf, again.buf) and torch.equal(first.columns, again.columns) and int(first.totals.sum()) > 0
    counts = PSDSCounts(3, NC, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        psds_counts(dev, ref, thr, win, PTR, counts=counts)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        psds_counts(dev, ref, thr, win, PTR, counts=counts)
    for _ in range(2):
        counts.buf.zero_()
        graph.replay()
        assert torch.equal(counts.buf, first.buf)

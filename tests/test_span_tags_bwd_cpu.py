"""CPU tests of the training path on span-level tags: the float64 statement of sed_stitch_span_tags_backward
(tests/span_tags_bwd_np.py) against central finite differences and against the recording-level statement, the host argument
checks of inference.pooled_span_tags and train.train_span_tags, and the epoch's plan of runs."""
import numpy as np
import pytest
import torch

from tests import span_tags_bwd_np, span_tags_np, stitch_np, weak_bwd_np
from tests.long_util import _n_windows

T3 = 8
L3S = [1, 5, 8, 9, 23]
NC = 3


def _tables(L3s, hop3):
    return (np.r_[0, np.cumsum([_n_windows(L, T3, hop3) for L in L3s])].astype(np.int32), np.r_[0, np.cumsum(L3s)].astype(np.int64))


def _inputs(hop3, weighting):
    rec_win0, rec_frame0 = _tables(L3S, hop3)
    rs = np.random.RandomState(300 + 10 * hop3 + weighting)
    n_win = int(rec_win0[-1])
    p = rs.uniform(0.02, 0.98, size=(n_win, T3, NC)).astype(np.float32)
    a = rs.uniform(0.05, 1.0, size=(n_win, T3, NC)).astype(np.float32)
    return rec_win0, rec_frame0, p, a, rs


@pytest.mark.parametrize("span3", [1, 3, 7, 8, 23])
@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", [1, 3, 8])
def test_statement_matches_central_finite_differences(hop3, weighting, span3):
    """d/dx of sum(g * tags) by central differences of the all-float64 pooling per span (span_tags_bwd_np.forward64, step
    1e-6) against the statement.  The recording-level bound 5e-6 |fd| + 1e-9 does not hold for spans: a short span's den is
    small, and the float32 rounding of the blended P and A (a half-ulp of a value <= 1 each, 2^-25) enters
    dA = g (P - t) / den absolutely.  Per element the bound is
        5e-6 |fd| + 1e-9 + 2^-22 |g[row, c]| (w / W) / den[row, c]
    - the last term four float32 half-ulps of values <= 1 carried through the formula.  A perturbed window element belongs to
    one recording, so the difference is taken of that recording's part of the sum (forward64 on its own tables: the other
    recordings' terms cancel exactly and would only add rounding).  Measured on this grid: the worst element sits at 0.20 of
    the bound (hop3 = 1, taper, span3 = 7; printed per case)."""
    rec_win0, rec_frame0, p, a, rs = _inputs(hop3, weighting)
    rec_span0 = span_tags_np.span_table(L3S, span3)
    g = rs.standard_normal((int(rec_span0[-1]), NC)).astype(np.float32)
    P = stitch_np.blend(p, rec_win0, rec_frame0, hop3, weighting)
    A = stitch_np.blend(a, rec_win0, rec_frame0, hop3, weighting)
    _, sums, _ = span_tags_np.pool_timelines(P, A, rec_frame0, span3)
    ds, da = span_tags_bwd_np.backward(p, a, rec_win0, rec_frame0, hop3, weighting, span3, g, sums=sums)

    h = 1e-6
    fd = [np.zeros(p.shape), np.zeros(p.shape)]
    for r, L3 in enumerate(L3S):
        w0, w1 = int(rec_win0[r]), int(rec_win0[r + 1])
        g_r = g[rec_span0[r]:rec_span0[r + 1]].astype(np.float64)
        t_w, t_f = np.array([0, w1 - w0], np.int32), np.array([0, L3], np.int64)
        x = [p[w0:w1].astype(np.float64), a[w0:w1].astype(np.float64)]

        def loss():
            return float((g_r * span_tags_bwd_np.forward64(x[0], x[1], t_w, t_f, hop3, weighting, span3)).sum())

        for k in range(2):
            for i in np.ndindex(*x[k].shape):
                keep = x[k][i]
                x[k][i] = keep + h
                up = loss()
                x[k][i] = keep - h
                dn = loss()
                x[k][i] = keep
                fd[k][(w0 + i[0],) + i[1:]] = (up - dn) / (2 * h)

    row, share = span_tags_bwd_np.frame_rows(rec_win0, rec_frame0, T3, hop3, weighting, span3)
    live = row >= 0
    extra = np.zeros(p.shape)
    extra[live] = 2.0 ** -22 * np.abs(g[row[live]].astype(np.float64)) * share[live][:, None] / sums[row[live], :, 1]
    worst = 0.0
    for name, got, want in (("d_win_strong", ds, fd[0]), ("d_win_att", da, fd[1])):
        bound = 5e-6 * np.abs(want) + 1e-9 + extra
        ratio = np.abs(got - want) / bound
        worst = max(worst, float(ratio.max()))
        print(f"hop3 {hop3} weighting {weighting} span3 {span3} {name}: max|statement - fd| {float(np.abs(got - want).max()):.3e}, "
              f"max|fd| {float(np.abs(want).max()):.3e}; worst element at {float(ratio.max()):.2f} of the bound")
    print(f"hop3 {hop3} weighting {weighting} span3 {span3}: worst ratio {worst:.3f}")
    for name, got, want in (("d_win_strong", ds, fd[0]), ("d_win_att", da, fd[1])):
        assert (np.abs(got - want) <= 5e-6 * np.abs(want) + 1e-9 + extra).all(), name
    # frames beyond a recording's end get no gradient: exactly +0.0
    zero = np.zeros(NC, np.float32).tobytes()
    for j, v in zip(*np.nonzero(~live)):
        assert ds[j, v].tobytes() == zero and da[j, v].tobytes() == zero
        assert (fd[0][j, v] == 0).all() and (fd[1][j, v] == 0).all()


@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", [1, 3, 8])
def test_one_span_per_recording_is_the_recording_level_statement(hop3, weighting):
    rec_win0, rec_frame0, p, a, rs = _inputs(hop3, weighting)
    g = rs.standard_normal((len(L3S), NC)).astype(np.float32)
    g[1] = 0.0
    ds, da = span_tags_bwd_np.backward(p, a, rec_win0, rec_frame0, hop3, weighting, 23, g)
    ws, wa = weak_bwd_np.backward(p, a, rec_win0, rec_frame0, hop3, weighting, g)
    assert ds.tobytes() == ws.tobytes() and da.tobytes() == wa.tobytes()
    assert np.abs(ds).max() > 0 and np.abs(da).max() > 0


def test_pooled_span_tags_checks_its_arguments_on_the_host():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.inference import pooled_span_tags
    p, a = torch.zeros(3, 8, 10), torch.ones(3, 8, 10)
    w0, f0 = torch.tensor([0, 1, 3], dtype=torch.int32), torch.tensor([0, 8, 20], dtype=torch.int64)
    with pytest.raises(ValueError, match="weighting"):
        pooled_span_tags(p, a, w0, f0, 20, 4, 5, weighting="linear")
    with pytest.raises(ValueError, match="n_win, T3, nclass"):
        pooled_span_tags(p, a[:2], w0, f0, 20, 4, 5)
    with pytest.raises(ValueError, match="n_win, T3, nclass"):
        pooled_span_tags(p[0], a[0], w0, f0, 20, 4, 5)
    for kw in (dict(hop3=0), dict(hop3=9), dict(total=0)):
        with pytest.raises(ValueError, match="need 1 <= nclass"):
            pooled_span_tags(p, a, w0, f0, kw.get("total", 20), kw.get("hop3", 4), 5)
    with pytest.raises(ValueError, match="need 1 <= nclass"):
        pooled_span_tags(torch.zeros(3, 8, 17), torch.zeros(3, 8, 17), w0, f0, 20, 4, 5)
    with pytest.raises(ValueError, match="need 1 <= nclass"):
        pooled_span_tags(p, a, w0[:1], f0[:1], 20, 4, 5)
    with pytest.raises(ValueError, match="2\\^31"):
        pooled_span_tags(p, a, w0, f0, 2 ** 31 // 10 + 1, 4, 5)
    with pytest.raises(ValueError, match="tables describe 4 windows"):
        pooled_span_tags(p, a, w0, f0, 20, 4, 5, n_win=4)
    with pytest.raises(_lib.SedError, match="GPU tensors"):
        pooled_span_tags(p, a, w0, f0, 20, 4, 5)                                   # no CPU fallback


def _long_set():
    from dcase2019_task4_amd.longrec import LongRecordingSet
    rs = np.random.RandomState(0)
    feats = [rs.standard_normal((n, 4)).astype(np.float32) for n in (64, 96, 128, 64, 128, 96)]
    return LongRecordingSet.from_arrays(feats, 64, hop_frames=32, device="cpu")


def test_train_span_tags_checks_its_arguments_on_the_host():
    from dcase2019_task4_amd.inference import span_table
    from dcase2019_task4_amd.train import train_span_tags
    s = _long_set()
    total = span_table(s, 4)[2]
    ok = np.zeros((total, 10), np.float32)
    with pytest.raises(ValueError, match="LongRecordingSet"):
        train_span_tags([1, 2], ok, None, None, 0, span3=4)
    with pytest.raises(ValueError, match="exactly one of tag_span"):
        train_span_tags(s, ok, None, None, 0)
    with pytest.raises(ValueError, match="exactly one of tag_span"):
        train_span_tags(s, ok, None, None, 0, tag_span=1.0, span3=4)
    with pytest.raises(ValueError, match="tag_span must be > 0"):
        train_span_tags(s, ok, None, None, 0, tag_span=0.0)
    with pytest.raises(ValueError, match="span3 must be"):
        train_span_tags(s, ok, None, None, 0, span3=0)
    with pytest.raises(ValueError, match=f"total_spans = {total}"):
        train_span_tags(s, ok[:-1], None, None, 0, span3=4)
    with pytest.raises(ValueError, match="total_spans"):
        train_span_tags(s, ok, None, None, 0, span3=3)
    with pytest.raises(ValueError, match="total_spans"):
        train_span_tags(s, ok[:, 0], None, None, 0, span3=4)
    for bad in (-0.1, 1.5, np.inf):
        t = ok.copy()
        t[3, 2] = bad
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            train_span_tags(s, t, None, None, 0, span3=4)
    with pytest.raises(ValueError, match="no known target"):
        train_span_tags(s, np.full_like(ok, np.nan), None, None, 0, span3=4)
    with pytest.raises(ValueError, match="more than max_windows"):
        train_span_tags(s, ok, None, None, 0, span3=4, max_windows=2)


def test_the_plan_skips_a_run_without_a_known_pair():
    from dcase2019_task4_amd.inference import span_table
    from dcase2019_task4_amd.train import recording_tag_batches, span_tag_plan
    s = _long_set()
    host, _, total, span3 = span_table(s, 4)
    n_w = np.diff(s.rec_win0_host)
    runs = recording_tag_batches(n_w, 4, 0, 0)[0]
    assert len(runs) >= 3
    t = np.random.RandomState(1).uniform(0, 1, size=(total, 10)).astype(np.float32)
    r0, r1 = runs[1]
    t[host[r0]:host[r1]] = np.nan                                                  # run 1: nothing known
    q0 = runs[2][0]
    t[host[q0]:host[q0 + 1], :] = np.nan
    t[host[q0], 3] = 0.25                                                          # run 2: one known pair
    plan = span_tag_plan(s.rec_win0_host, s.rec_frame0_host, t, 4, 4)
    assert plan["runs"] == runs and plan["total_spans"] == total and plan["span3"] == span3
    assert plan["rec_span0"].tolist() == host.tolist()
    assert plan["ran"] == [k for k in range(len(runs)) if k != 1]
    assert plan["counts"][1] == 0
    assert plan["counts"][0] == (host[runs[0][1]] - host[runs[0][0]]) * 10
    assert plan["counts"][2] == 1 + (host[runs[2][1]] - host[q0 + 1]) * 10
    assert plan["counts"].sum() == int((~np.isnan(t)).sum())
    assert plan["known"].tobytes() == (~np.isnan(t)).astype(np.float32).tobytes()
    assert not np.isnan(plan["targets"]).any() and (plan["targets"][plan["known"] == 1] == t[~np.isnan(t)]).all()
    # an "infinite" span is one span per recording: the recording-level layout
    plan = span_tag_plan(s.rec_win0_host, s.rec_frame0_host, np.zeros((s.n_rec, 10), np.float32), 4, np.inf)
    assert plan["rec_span0"].tolist() == list(range(s.n_rec + 1)) and plan["span3"] == int(np.diff(s.rec_frame0_host).max())

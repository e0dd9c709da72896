"""CPU tests of the training path on recording-level tags: the float64 statement of sed_stitch_weak_backward
(tests/weak_bwd_np.py) against central finite differences, the host argument checks of inference.pooled_tags, and the batch
packing of train.train_recording_tags."""
import numpy as np
import pytest
import torch

from tests import weak_bwd_np
from tests.long_util import _n_windows

T3 = 8
L3S = [1, 5, 8, 9, 23]


def _tables(L3s, hop3):
    return (np.r_[0, np.cumsum([_n_windows(L, T3, hop3) for L in L3s])].astype(np.int32), np.r_[0, np.cumsum(L3s)].astype(np.int64))


@pytest.mark.parametrize("weighting", [0, 1])
@pytest.mark.parametrize("hop3", [1, 3, 8])
def test_statement_matches_central_finite_differences(hop3, weighting):
    """d/dx of sum(g * weak) by central differences of the all-float64 pooling (weak_bwd_np.forward64, step 1e-6: truncation
    ~1e-12, cancellation ~1e-10) against the statement, which differs from it by the float32 rounding of the blend (2^-24
    relative on P and A) and of its own float32 outputs.  Every element within 5e-6 relative + 1e-9 of its finite difference.
    Measured on this grid (every element of every window, tails included): the worst element is at 0.79 of that bound
    (d_win_att, hop3 = 1, taper), and the largest difference of a tensor is 5e-8 of the tensor's largest element; the 7e-7
    of the four-length subset was not reproduced."""
    NC = 3
    rec_win0, rec_frame0 = _tables(L3S, hop3)
    rs = np.random.RandomState(300 + 10 * hop3 + weighting)
    n_win = int(rec_win0[-1])
    p = rs.uniform(0.02, 0.98, size=(n_win, T3, NC)).astype(np.float32)
    a = rs.uniform(0.05, 1.0, size=(n_win, T3, NC)).astype(np.float32)
    g = rs.standard_normal((len(L3S), NC)).astype(np.float32)
    ds, da = weak_bwd_np.backward(p, a, rec_win0, rec_frame0, hop3, weighting, g)

    def loss(pp, aa):
        return float((g.astype(np.float64) * weak_bwd_np.forward64(pp, aa, rec_win0, rec_frame0, hop3, weighting)).sum())

    h = 1e-6
    fd = [np.zeros(p.shape), np.zeros(p.shape)]
    x = [p.astype(np.float64), a.astype(np.float64)]
    for k in range(2):
        for i in np.ndindex(*p.shape):
            keep = x[k][i]
            x[k][i] = keep + h
            up = loss(*x)
            x[k][i] = keep - h
            dn = loss(*x)
            x[k][i] = keep
            fd[k][i] = (up - dn) / (2 * h)
    for name, got, want in (("d_win_strong", ds, fd[0]), ("d_win_att", da, fd[1])):
        err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
        ratio = float((np.abs(got - want) / (5e-6 * np.abs(want) + 1e-9)).max())
        print(f"hop3 {hop3} weighting {weighting} {name}: max|statement - fd| {err:.3e}, max|fd| {scale:.3e}, ratio {err / scale:.3e}; "
              f"worst element at {ratio:.2f} of 5e-6 relative + 1e-9")
        np.testing.assert_allclose(got, want, rtol=5e-6, atol=1e-9, err_msg=name)
    # frames beyond a recording's end get no gradient: exactly +0.0
    for r, L3 in enumerate(L3S):
        for j in range(int(rec_win0[r + 1] - rec_win0[r])):
            for v in range(T3):
                if j * hop3 + v >= L3:
                    for arr in (ds, da):
                        assert arr[rec_win0[r] + j, v].tobytes() == np.zeros(NC, np.float32).tobytes()
                    assert (fd[0][rec_win0[r] + j, v] == 0).all() and (fd[1][rec_win0[r] + j, v] == 0).all()


def test_pooled_tags_checks_its_arguments_on_the_host():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.inference import pooled_tags
    p, a = torch.zeros(3, 8, 10), torch.ones(3, 8, 10)
    w0, f0 = torch.tensor([0, 1, 3], dtype=torch.int32), torch.tensor([0, 8, 20], dtype=torch.int64)
    with pytest.raises(ValueError, match="weighting"):
        pooled_tags(p, a, w0, f0, 20, 4, weighting="linear")
    with pytest.raises(ValueError, match="n_win, T3, nclass"):
        pooled_tags(p, a[:2], w0, f0, 20, 4)
    with pytest.raises(ValueError, match="n_win, T3, nclass"):
        pooled_tags(p[0], a[0], w0, f0, 20, 4)
    for kw in (dict(hop3=0), dict(hop3=9), dict(total=0)):
        with pytest.raises(ValueError, match="need 1 <= nclass"):
            pooled_tags(p, a, w0, f0, kw.get("total", 20), kw.get("hop3", 4))
    with pytest.raises(ValueError, match="need 1 <= nclass"):
        pooled_tags(torch.zeros(3, 8, 17), torch.zeros(3, 8, 17), w0, f0, 20, 4)
    with pytest.raises(ValueError, match="need 1 <= nclass"):
        pooled_tags(p, a, w0[:1], f0[:1], 20, 4)
    with pytest.raises(ValueError, match="2\\^31"):
        pooled_tags(p, a, w0, f0, 2 ** 31 // 10 + 1, 4)
    with pytest.raises(ValueError, match="tables describe 4 windows"):
        pooled_tags(p, a, w0, f0, 20, 4, n_win=4)
    with pytest.raises(_lib.SedError, match="GPU tensors"):
        pooled_tags(p, a, w0, f0, 20, 4)                                       # no CPU fallback


def test_recording_tag_batches_are_consecutive_runs_within_max_windows():
    from dcase2019_task4_amd.train import recording_tag_batches
    rs = np.random.RandomState(4)
    for max_windows in (5, 7, 64):
        n_w = rs.randint(1, 6, size=40)
        runs, order = recording_tag_batches(n_w, max_windows, 3, 0)
        assert runs[0][0] == 0 and runs[-1][1] == len(n_w)
        assert all(a[1] == b[0] for a, b in zip(runs, runs[1:])) and all(r1 > r0 for r0, r1 in runs)
        assert all(n_w[r0:r1].sum() <= max_windows for r0, r1 in runs)
        # greedy: the next recording would not have fitted
        assert all(n_w[r0:r1].sum() + n_w[r1] > max_windows for r0, r1 in runs[:-1])
        assert sorted(order.tolist()) == list(range(len(runs)))
    assert recording_tag_batches([2, 2, 2], 64, 0, 0)[0] == [(0, 3)]
    assert recording_tag_batches([3, 3, 3], 3, 0, 0)[0] == [(0, 1), (1, 2), (2, 3)]


def test_recording_tag_batch_order_is_a_function_of_seed_and_epoch():
    from dcase2019_task4_amd.train import recording_tag_batches
    n_w = [2] * 40
    runs, o00 = recording_tag_batches(n_w, 4, 0, 0)
    assert len(runs) == 20
    assert recording_tag_batches(n_w, 4, 0, 0)[1].tolist() == o00.tolist()
    assert o00.tolist() == np.random.default_rng([0, 0]).permutation(20).tolist()
    o01, o10 = recording_tag_batches(n_w, 4, 0, 1)[1], recording_tag_batches(n_w, 4, 1, 0)[1]
    assert o01.tolist() != o00.tolist() and o10.tolist() != o00.tolist() and o10.tolist() != o01.tolist()
    assert recording_tag_batches(n_w, 4, 0, 1)[0] == runs                         # the runs do not depend on either


def test_a_recording_over_max_windows_is_refused():
    from dcase2019_task4_amd.train import recording_tag_batches
    with pytest.raises(ValueError, match="recording 2 has 9 windows"):
        recording_tag_batches([1, 8, 9, 2], 8, 0, 0)
    with pytest.raises(ValueError):
        recording_tag_batches([], 8, 0, 0)

"""-m gpu: the train forward and backward against the oracle at the shapes that sit on the edges of the prologue loads of
k_x_moments, k_glu_pool_fwd, k_glu_pool_bwd8, k_blk0_bwd_finalize and the dgrad k_conv_wino: loads that are issued from clamped
addresses ahead of the condition that says whether their value is used, and zeroed or dropped afterwards.  A wrong clamp or a
dropped zeroing shows here as a wrong posterior, BatchNorm statistic or gradient; the tolerances are those of
tests/test_gpu_parity.py::test_train_forward_backward_vs_oracle, whose helpers do the work."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu, synth
from tests import gpu_util as gu
from tests import test_gpu_parity as par

pytestmark = pytest.mark.gpu


def _target(B, T_out, nclass=10):
    """synth.make_target's [weak | unlabeled | strong] layout with labelled rows at any batch size: make_target gives B // 4 weak
    and strong rows, none below B = 4, and the class loss over no rows is NaN on both sides - which would compare nothing.
    Here: max(B // 4, 1) weak rows at the front, as many strong rows at the back (the same row at B = 1), the rest unlabeled."""
    rs = np.random.RandomState(3005)
    n = max(B // 4, 1)
    t = np.full((B, T_out, nclass), -1.0)
    t[:n] = (rs.uniform(size=(n, 1, nclass)) < 0.2).astype(np.float64)
    t[B - n:] = (rs.uniform(size=(n, T_out, nclass)) < 0.2).astype(np.float64)
    return torch.tensor(t, dtype=torch.float32), slice(n), slice(B - n, B)


def _fwd_bwd_both(B, T, p, seed):
    """test_gpu_parity._fwd_bwd_both on _target's labels."""
    model, params = gu.make_model(0, dropout=p)
    model.train()
    x = synth.make_input(40, B, T)
    tgt, wm, sm = _target(B, T // 8)
    rs = np.random.RandomState(99)
    s_ema = torch.tensor(rs.uniform(0.05, 0.95, (B, T // 8, 10)), dtype=torch.float32)
    w_ema = torch.tensor(rs.uniform(0.05, 0.95, (B, 10)), dtype=torch.float32)

    def loss_fn(s, w, dev):
        return ref_cpu.mean_teacher_loss(s, w, s_ema.to(dev), w_ema.to(dev), tgt.to(dev), wm, sm, 0.7)[0]

    s, w = model(x.cuda(), seed=gu.seed_tensor(seed))
    loss = loss_fn(s, w, "cuda")
    loss.backward()
    torch.cuda.synchronize()
    g_hip, bn_hip = gu.grads_dict(model), gu.bn_state_from_model(model)
    po = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    bn = ref_cpu.new_bn_state()
    so, wo = ref_cpu.crnn_forward(po, x, True, bn, gu.oracle_masks(seed, B, T, p))
    lo = loss_fn(so, wo, "cpu")
    go = dict(zip(po.keys(), torch.autograd.grad(lo, list(po.values()))))
    return (s.detach().cpu(), w.detach().cpu(), float(loss.detach()), g_hip, bn_hip), (so.detach(), wo.detach(), float(lo.detach()), go, bn)


@pytest.mark.parametrize("B,T", [(1, 24), (2, 64), (3, 65), (2, 136)])
def test_train_forward_backward_vs_oracle_on_the_edges_of_the_prologue_loads(B, T):
    """(1, 24): block 2 has Q = 3 pooled pixels - less than one row block (the y tile's rows past Q read the clamped pixel) -
    block 1 has 6 row blocks, so the last workgroup has idle waves, and the one moments tile ends far short of its 64 rows.
    (2, 64): the moments tile is exactly full and its lower halo row is out of range (clamped row, zeroed).
    (3, 65): a second moments tile holds one row; T is odd.
    (2, 136): 17 GRU steps, block-2 H = 34 and block-1 H = 68, the last moments tile partial.
    Checks and tolerances: those of test_gpu_parity.test_train_forward_backward_vs_oracle."""
    hip, orc = _fwd_bwd_both(B, T, 0.5, seed=123456789)
    es, _ = gu.report("strong", hip[0], orc[0])
    ew, _ = gu.report("weak", hip[1], orc[1])
    assert es < par.POST_TOL and ew < par.POST_TOL
    assert np.isfinite(orc[2]) and hip[2] == pytest.approx(orc[2], rel=1e-5)
    par._check_grads(hip[3], orc[3])
    for k, v in orc[4].items():
        np.testing.assert_allclose(hip[4][k].numpy(), v.numpy(), rtol=3e-5, atol=3e-6, err_msg=k)


def test_the_step_is_bit_identical_eager_and_replayed_at_an_odd_shape():
    """The same mean-teacher steps at (3, 65), launched eagerly and replayed as a hipGraph: the load order inside a kernel
    changes nothing about what it computes, whatever runs beside it - gradients and posteriors agree to the bit after each of
    four steps (the later ones start from the earlier ones' Adam updates)."""
    from dcase2019_task4_amd.train import MeanTeacherStep
    B, T, steps = 3, 65, 4
    tgt, wm, sm = _target(B, T // 8)
    x, xe = synth.make_input(60, B, T).cuda(), synth.make_input(70, B, T).cuda()
    res = {}
    for graph in (False, True):
        s, _ = gu.make_model(0, dropout=0.5)
        t, _ = gu.make_model(1, dropout=0.5)
        s.train(); t.train()
        st = MeanTeacherStep(s, t, B, T, 150, wm, sm, seed=99, use_graph=graph)
        out = []
        for _ in range(steps):
            st.load_batch(x, xe, tgt.cuda())
            st.run()
            torch.cuda.synchronize()
            out.append((st.grads.clone(), st.strong.clone(), st.weak.clone()))
        st.check_health()
        assert bool(st._graph_sets) == graph           # steps 3 and 4 were replays
        res[graph] = out
        st.close()
    for k, (a, b) in enumerate(zip(res[False], res[True])):
        assert torch.isfinite(a[0]).all() and float(a[0].abs().max()) > 0
        for name, u, v in zip(("grads", "strong", "weak"), a, b):
            assert torch.equal(u, v), (k, name, float((u - v).abs().max()))

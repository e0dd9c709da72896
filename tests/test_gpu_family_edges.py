"""-m gpu parity tests of the GENERIC kernel set (csrc/gen.h) at the shapes where kernels go wrong: the reduced-precision modes
(bf16, f16, bf16x3) and the wide / mixed fp32 geometries at T < 128, odd T, B = 1 in train mode, the ABI's minimum T, nclass 1
and 16 and one GRU layer - posteriors, loss, every gradient and the BatchNorm statistics against the CPU oracle on identical
inputs and Philox masks, each at the bound tests/test_gpu_generic.py applies to that mode and geometry (gradients of the
cases in EDGE_CASES: at measured bounds of their own, see there).

Why small shapes: the family's gradient bounds (worst element <= 0.14 / 0.09 of the gradient's rms) cannot see a dropped border
row at T = 628 - one row of 157 in a weight-gradient sum is under 1 %.  At T = 22 the image is 22 -> 11 -> 5 -> 2 rows: a border
row is a fifth to a tenth of every sum, and the same bounds do see it.  That the ARITHMETIC alone stays inside the posterior
bounds at these shapes was checked on the CPU (tests/bf16_budget.py's rounding-injected forward, every operator rounding, inputs
x and 2 x + 0.5): f16 <= 1.6e-4 against 1e-3, bf16 base <= 4.6e-4 against 1.3e-3, bf16 wide <= 1.0e-3 against 3e-3."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu, synth
from tests import gpu_util as gu
from tests.test_gpu_generic import (BF16_GRAD_TOL, BF16_POST_TOL, BF16_POST_TOL_BASE, F16_GRAD_TOL, F16_POST_TOL, POST_TOL,
                                    X3_GRAD_TOL, X3_POST_TOL, _grad_errors, _stage_report)

pytestmark = pytest.mark.gpu

SEED = 987654321
BASE, WIDE = (64, 64), (128, 256)
# (B, T, p): (3, 22) every pool floor drops a row from block 1 on, 2 GRU steps; (1, 29) odd T - the first pool drops an input
# row - and B = 1; (5, 16) the ABI's minimum T (a 2-row image in block 2), the byte-per-element dropout stream; (2, 45) an odd
# height at every stage (45 -> 22 | 22 -> 11 | 11 -> 5)
SHAPES = [(3, 22, 0.5), (1, 29, 0.5), (5, 16, 0.25), (2, 45, 0.5)]
_ORACLE = {}

# Gradient bounds of their own for the cases that exceed the shared constants (profiles/edge_shape_gradient_errors.md has every
# figure).  Ruled out as a kernel fault before any of them was set: at the same shapes f32 and bf16x3 hold THEIR bounds with
# room (worst element <= 2e-4 of the rms - no row, frame or clip is dropped), and the Frobenius-relative error of every tensor
# in bf16 / f16, measured at (3, 22) wide, is 6e-4 .. 8e-3 as it is at B = 48 (one term dropped from a 3 .. 10-term sum would
# be >= 0.3).  What moves is the statistic: with B x T / 8 = 3 .. 10 terms per weight-gradient sum the gradient tensors are
# heavy-tailed (largest element of the layer-1 reverse weights 26 - 27 rms at (3, 22) wide against 14 - 15 at B = 48), and the
# rounding of bf16 operands (2^-8 .. 2^-7) on terms that large is 0.1 - 0.2 rms wherever it lands - 0.47 % of a 24-rms element
# is 0.11 rms.  The metric falls back inside the shared bounds as B grows at the same T (wide bf16 recurrences 0.19 / 0.10 / 0.08
# at B = 3 / 12 / 48; wide f16 0.11 / 0.03 at B = 3 / 48).
# Measured maximum over the listed cases + 35 %, and never above twice the shared constant - which is what binds for the f16
# recurrences (*): measured 6.65e-2 (H = 64) and 1.13e-1 (H = 256; weight_hh_l1_reverse at (3, 22), the same figure to every
# printed digit in both runs that measured it).
#   bf16 wide, recurrences + heads   1.94e-1 (weight_ih_l1_reverse at (3, 22); heads 1.84e-1 with one GRU layer)   shared 1.4e-1
#   f16 heads, wide (5, 16)          1.05e-2                                                                        shared 7.8e-3
EDGE_BF16_GRAD_TOL = 2.6e-1
EDGE_F16_GRAD_TOL = {"rnn64": 7.2e-2, "rnn256": 1.14e-1, "heads": 1.42e-2}          # (*) rnn64, rnn256: 2 x F16_GRAD_TOL
assert EDGE_BF16_GRAD_TOL <= 2 * BF16_GRAD_TOL
assert all(v <= 2 * F16_GRAD_TOL[k] + 1e-12 for k, v in EDGE_F16_GRAD_TOL.items())
# (dtype, (C, H), B, T, variant) -> the layer classes that take the edge bound there; every other class of these cases, and every
# class of every other case, is held to the shared constant
EDGE_CASES = {
    ("bf16", WIDE, 3, 22, ""): ("rnn",), ("bf16", WIDE, 3, 22, "nclass1"): ("rnn",),
    ("bf16", WIDE, 3, 22, "one_gru_layer"): ("rnn", "heads"),
    ("f16", BASE, 3, 22, ""): ("rnn",), ("f16", BASE, 1, 29, ""): ("rnn",), ("f16", BASE, 3, 22, "nclass1"): ("rnn",),
    ("f16", BASE, 3, 22, "nclass16"): ("rnn",), ("f16", BASE, 3, 22, "one_gru_layer"): ("rnn",),
    ("f16", WIDE, 3, 22, ""): ("rnn",), ("f16", WIDE, 1, 29, ""): ("rnn",), ("f16", WIDE, 5, 16, ""): ("rnn", "heads"),
}


def _problem(B, T, nclass):
    """Input, target and teacher outputs of one case.  Every clip is strongly labelled; the weak and the strong mask each cover
    half of the batch (rounded up, so that neither is empty at B = 1: synth.make_target gives B < 4 no labelled clip)."""
    x = synth.make_input(40, B, T)
    rs = np.random.RandomState(99)
    tgt = torch.tensor((rs.uniform(size=(B, T // 8, nclass)) < 0.2).astype(np.float32))
    s_ema = torch.tensor(rs.uniform(0.05, 0.95, (B, T // 8, nclass)), dtype=torch.float32)
    w_ema = torch.tensor(rs.uniform(0.05, 0.95, (B, nclass)), dtype=torch.float32)
    wm, sm = slice(0, (B + 1) // 2), slice(B // 2, B)

    def loss_fn(s, w, dev):
        return ref_cpu.mean_teacher_loss(s, w, s_ema.to(dev), w_ema.to(dev), tgt.to(dev), wm, sm, 0.7)[0]

    return x, loss_fn


def _oracle(B, T, p, C, H, n_layers, nclass):
    """The fp32 oracle of one case: computed once, shared by every arithmetic mode, never written to."""
    key = (B, T, p, C, H, n_layers, nclass)
    if key not in _ORACLE:
        x, loss_fn = _problem(B, T, nclass)
        params = synth.make_params(0, n_layers_RNN=n_layers, nclass=nclass, nb_filters=(C,) * 3, n_RNN_cell=H)
        po = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        bn = ref_cpu.new_bn_state([C] * 3)
        so, wo, inter = ref_cpu.crnn_forward(po, x, True, bn, gu.oracle_masks(SEED, B, T, p, C, H), n_layers_RNN=n_layers,
                                             return_intermediates=True)
        lo = loss_fn(so, wo, "cpu")
        go = dict(zip(po.keys(), torch.autograd.grad(lo, list(po.values()))))
        _ORACLE[key] = dict(so=so.detach(), wo=wo.detach(), lo=float(lo.detach()), go=go, bno=bn,
                            inter={k: v.detach() for k, v in inter.items()})
    return _ORACLE[key]


def _run(dtype, C, H, B, T, p, n_layers=2, nclass=10):
    ora = _oracle(B, T, p, C, H, n_layers, nclass)
    model, _ = gu.make_model(0, dropout=p, n_layers=n_layers, nclass=nclass, C=C, H=H, mfma_dtype=dtype)
    model.train()
    x, loss_fn = _problem(B, T, nclass)
    s, w = model(x.cuda(), seed=gu.seed_tensor(SEED))
    loss = loss_fn(s, w, "cuda")
    loss.backward()
    torch.cuda.synchronize()
    _stage_report(model, ora["inter"], B, T, C, H)
    if H == 256:      # the cluster recurrence's bounded spins never timed out
        assert int(model.ctx_view("gru_err").view(torch.int32)[0]) == 0
    return dict(ora, s=s.detach().cpu(), w=w.detach().cpu(), loss=float(loss.detach()), g=gu.grads_dict(model),
                bn=gu.bn_state_from_model(model))


def _check(r, dtype, C, H, B, T, variant=""):
    """The assertions of test_gpu_generic.py's test of this mode, bounds unchanged - but for the gradient bounds of the layer
    classes EDGE_CASES lists."""
    es, _ = gu.report(f"strong ({dtype})", r["s"], r["so"])
    ew, _ = gu.report(f"weak ({dtype})", r["w"], r["wo"])
    cls = {}
    worst, name = _grad_errors(r["g"], r["go"], cls)
    print(f"[edges {dtype}] C={C} H={H} B={B} T={T} {variant}: posterior err strong {es:.2e} weak {ew:.2e}; loss {r['loss']:.6f} / "
          f"{r['lo']:.6f}; worst gradient err/typ {worst:.2e} ({name}); per class " +
          " ".join(f"{k} {v:.2e}" for k, v in sorted(cls.items())))
    assert torch.isfinite(r["s"]).all() and torch.isfinite(r["w"]).all()
    if dtype == "f32":
        post, loss_rel, bn_tol = POST_TOL, 1e-5, dict(rtol=3e-5, atol=3e-6)
    elif dtype == "bf16":
        post, loss_rel, bn_tol = (BF16_POST_TOL_BASE if (C, H) == BASE else BF16_POST_TOL), 5e-3, dict(rtol=2e-2, atol=5e-3)
    elif dtype == "bf16x3":
        post, loss_rel, bn_tol = X3_POST_TOL, 1e-4, dict(rtol=1e-3, atol=1e-4)
    else:
        post, loss_rel, bn_tol = F16_POST_TOL, 1e-3, dict(rtol=4e-3, atol=1e-3)
    assert es < post and ew < post, (es, ew, post)
    assert r["loss"] == pytest.approx(r["lo"], rel=loss_rel)
    edge = EDGE_CASES.get((dtype, (C, H), B, T, variant), ())
    assert dtype in ("bf16", "f16") or not edge
    for k in ("cnn", "rnn", "heads"):
        if dtype == "f16":
            key = "rnn%d" % H if k == "rnn" else k
            tol = EDGE_F16_GRAD_TOL[key] if k in edge else F16_GRAD_TOL[key]
        elif dtype == "bf16":
            tol = EDGE_BF16_GRAD_TOL if k in edge else BF16_GRAD_TOL
        else:
            tol = {"f32": 1e-3, "bf16x3": X3_GRAD_TOL}[dtype]
        assert cls[k] < tol, (k, tol, name, cls)
    for k, v in r["bno"].items():
        if dtype == "f32" or not k.endswith("num_batches_tracked"):
            np.testing.assert_allclose(r["bn"][k].numpy(), v.numpy(), err_msg=k, **bn_tol)


@pytest.mark.parametrize("B,T,p", SHAPES)
@pytest.mark.parametrize("C,H", [BASE, WIDE])
@pytest.mark.parametrize("dtype", ["bf16", "f16", "bf16x3"])
def test_reduced_precision_modes_at_edge_shapes(dtype, C, H, B, T, p):
    _check(_run(dtype, C, H, B, T, p), dtype, C, H, B, T)


@pytest.mark.parametrize("B,T,p", [(1, 29, 0.5), (5, 16, 0.25)])
@pytest.mark.parametrize("C,H", [WIDE, (128, 64), (64, 256)])
def test_generic_fp32_at_edge_shapes(C, H, B, T, p):
    """The generic set in exact fp32 - the wide geometry and the two mixed ones - at the specialised set's bounds."""
    _check(_run("f32", C, H, B, T, p), "f32", C, H, B, T)


@pytest.mark.parametrize("variant", ["nclass1", "nclass16", "one_gru_layer"])
@pytest.mark.parametrize("dtype,C,H", [("f16", *BASE), ("bf16", *WIDE)])
def test_head_and_recurrence_variants_at_22_frames(dtype, C, H, variant):
    """nclass 1 and 16 (the ABI's limits) and n_layers_RNN = 1 (the CRNN constructor's default) at (3, 22)."""
    kw = {"nclass1": dict(nclass=1), "nclass16": dict(nclass=16), "one_gru_layer": dict(n_layers=1)}[variant]
    _check(_run(dtype, C, H, 3, 22, 0.5, **kw), dtype, C, H, 3, 22, variant)

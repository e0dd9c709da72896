"""-m gpu: the output heads and the mean-teacher loss at CONFIDENT posteriors.  Every other parity test drives them with a randomly
initialised model - strong in 0.40 .. 0.61, no attention value near the 1e-7 clamp -, so neither BCELoss's clamps (log at -100,
gradient denominator at 1e-12), nor the fast sigmoid beyond |z| = 2, nor the clamp's pass mask, nor a class whose attention is
clamped in every frame, nor the edges of the label groups ever had a side that could fail.  Here the head parameters alone are
steered (tests/gpu_util.steer_heads: "ladder" = exact saturation, "confident" = no cliff) and the kernels are held to the plain
float64 statement tests/heads_np.py, to the float32 / float64 oracle, and to each other (the three forms of the loss).

Shapes: (2, 16), (3, 136), (2, 1040) give T / 8 = 2, 17 and 130 frames - the last more than one 128-frame chunk, so not fused
into the backward recurrence -, (2, 264) on the wide model (C = 128 / H = 256) 33 frames, one past a 32-frame chunk of its heads
kernels.  Measured figures: profiles/heads_regimes.md."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import philox, ref_cpu, synth
from tests import gpu_util as gu
from tests import heads_np
from tests import test_gpu_parity as tp

pytestmark = pytest.mark.gpu

WIDE = dict(C=128, H=256)
SHAPES = [(2, 16, {}), (3, 136, {}), (2, 1040, {}), (2, 264, WIDE)]
SHAPE_IDS = ["2x16", "3x136", "2x1040", "wide-2x264"]
DROP_SEED = 123456789
# Input seeds (synth.make_input) at which the guards below hold; every other case uses 40.  Modes: "train" = train mode with
# dropout 0.5 under DROP_SEED, "train0" = train mode without dropout, "eval".  The ladder is 80 % off the clamp at any seed.  The
# confident steering spreads its attention continuously across the clamp, so the margin shrinks with the number of values: the
# nearest one is 79 % off at (2, 16) train, 5 % / 11 % at (3, 136), 2.1 % at (2, 1040) eval and 1.3 % at (2, 1040) train0 (2600
# values, a fifth clamped).  tests/test_heads_regimes_cpu.py asserts these margins with the CPU oracle.  If a guard trips after a
# change to anything in front of the heads, nothing is wrong with the heads: pick another seed for that case with the CPU test
# (it runs the same forward) and pin it here.
X_SEED = {("confident", 2, 16, "eval"): 72, ("confident", 3, 136, "eval"): 67, ("confident", 2, 1040, "eval"): 54,
          ("confident", 2, 16, "train0"): 46, ("confident", 3, 136, "train0"): 60, ("confident", 2, 1040, "train0"): 148,
          ("confident", 2, 16, "train"): 45}
CONFIDENT_TRAIN_SHAPES = [(2, 16), (3, 136), (2, 1040)]            # train mode WITHOUT dropout
CONFIDENT_DROPOUT_SHAPES = [(2, 16)]                               # train mode with dropout 0.5: see FWD_CASES
U24 = 2.0 ** -24
SEPARATE_HEADS = 1 << 24


def _x_seed(steering, B, T, mode):
    return X_SEED.get((steering, B, T, mode), 40)


def _guards(raw, strong64, steering):
    """The inputs keep clear of the two places where a float32 kernel and a float64 statement may rightly disagree.  A guard
    that fails fails the test: no element is skipped."""
    assert (np.abs(raw / heads_np.ATT_MIN - 1.0) > 0.01).all(), \
        "an input guard, not a kernel error: a raw attention value within 1 % of the 1e-7 clamp - pin another input seed (X_SEED)"
    if steering == "confident":
        assert np.minimum(strong64, 1.0 - strong64).min() >= 1e-4, \
            "an input guard, not a kernel error: a strong posterior within 1e-4 of 0 or 1 - pin another input seed (X_SEED)"


def _target01(seed, B, T3, NC):
    rs = np.random.RandomState(3100 + seed)
    return torch.tensor((rs.uniform(size=(B, T3, NC)) < 0.3).astype(np.float32))


def _groups_for(B):
    """weak rows [0, B - 1), strong rows [1, B): overlapping for B >= 3."""
    return slice(0, B - 1), slice(1, B)


# ---- a. the loss kernel at hand-placed posteriors -------------------------------------------------------------------------------
P_SET = np.array([0.0, 2.0 ** -126, 1e-30, 1e-13, 1e-7, 0.5, 1.0 - 1e-6, 1.0 - 2.0 ** -24, 1.0], dtype=np.float32)


def _mt_loss_call(st, wlo, whi, slo, shi):
    from dcase2019_task4_amd import _lib
    _lib.check(st.l.sed_mt_loss(C.byref(st.dims), _lib.ptr(st.strong), _lib.ptr(st.weak), _lib.ptr(st.strong_ema),
                                _lib.ptr(st.weak_ema), _lib.ptr(st.target), wlo, whi, slo, shi,
                                _lib.ptr(st.state), _lib.ptr(st.losses), _lib.ptr(st.d_strong), _lib.ptr(st.d_weak),
                                _lib.stream_ptr()), "sed_mt_loss")
    torch.cuda.synchronize()


def _assert_loss_outputs(st, groups, tag):
    """meters, d_strong, d_weak of the step's buffers against the float64 statement on the values stored in them."""
    s, w, se, we, tgt = (t.cpu().numpy() for t in (st.strong, st.weak, st.strong_ema, st.weak_ema, st.target))
    m = st.meters()
    want, ds, dw = heads_np.mt_loss(s, w, se, we, tgt, *groups, m["cons_weight"])
    for name, got, ref in (("d_strong", st.d_strong.cpu().numpy(), ds), ("d_weak", st.d_weak.cpu().numpy(), dw)):
        assert np.isfinite(got).all(), (tag, name)
        nz = ref != 0
        big = np.abs(ref) > 1e-25                 # (below: float32 denormals of the consistency term, held by the absolute 1e-30)
        rel = np.abs(got[big] - ref[big]) / np.abs(ref[big])
        print(f"[heads regimes] {tag} {name}: max rel err {rel.max() if big.any() else 0.0:.3e} over {int(big.sum())} above 1e-25, "
              f"{int(nz.sum() - big.sum())} non-zero below, {int((~nz).sum())} exact zeros")
        assert (got[~nz] == 0.0).all(), (tag, name)
        # at most six fp32 operations and one division per element: ~1e-6
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-30, err_msg=f"{tag} {name}")
    for k, v in zip(heads_np.METERS[:7], want[:7]):
        assert np.isfinite(m[k]), (tag, k)
        assert m[k] == pytest.approx(v, rel=2e-5, abs=1e-9), (tag, k, m[k], v)
    wlo, whi, slo, shi = groups
    if whi == wlo:
        assert m["weak_class_loss"] == 0.0 and m["weak_ema_loss"] == 0.0, tag
    if shi == slo:
        assert m["strong_loss"] == 0.0 and m["strong_ema_loss"] == 0.0, tag
    return m


def hand_placed(B, T3, NC):
    """Posteriors of student and teacher cycling through P_SET, targets 0 / 1 in runs of nine, so that every (posterior, target)
    pair occurs in each labelled group (rows [0, 3) weak, [1, 4) strong) once there are enough elements (NC >= 10)."""
    i = np.arange(B * T3 * NC).reshape(B, T3, NC)
    j = np.arange(B * NC).reshape(B, NC)
    tgt = ((i // 9) % 2).astype(np.float32)
    bc = (np.arange(B)[:, None] + np.arange(NC)[None, :] + j // 9) % 2 == 1
    tgt[:3] *= ~bc[:3, None, :]                       # weak rows: about every second (row, class) has no active frame - a weak target of 0
    strong, strong_ema = P_SET[i % 9], P_SET[(i + i // 9) % 9]
    weak, weak_ema = P_SET[(j + 3) % 9], P_SET[(2 * j + j // 9) % 9]
    if NC >= 10:
        tw = tgt.max(1)
        assert len({(float(p), float(t)) for p, t in zip(strong[1:].ravel(), tgt[1:].ravel())}) == 18
        assert len({(float(p), float(t)) for p, t in zip(weak[:3].ravel(), tw[:3].ravel())}) == 18
    return strong, weak, strong_ema, weak_ema, tgt


@pytest.mark.parametrize("nclass", [1, 10, 16])
def test_loss_kernel_at_hand_placed_saturated_posteriors(nclass):
    """sed_mt_loss with student and teacher posteriors from {0, 2^-126, 1e-30, 1e-13, 1e-7, 0.5, 1 - 1e-6, 1 - 2^-24, 1} (clear of
    (1 - p) p within 1 % of 1e-12) against targets 0 / 1: both logarithm clamps, the gradient clamp on both sides, weak exactly 0
    and 1.  Rows [0, 3) weak, [1, 4) strong."""
    from dcase2019_task4_amd.train import MeanTeacherStep
    B, T, NC = 4, 136, nclass
    T3 = T // 8
    student, _ = gu.make_model(0, dropout=0, nclass=NC)
    teacher, _ = gu.make_model(1, dropout=0, nclass=NC)
    st = MeanTeacherStep(student, teacher, B, T, 150, slice(0, 3), slice(1, 4), use_graph=False)
    strong, weak, strong_ema, weak_ema, tgt = hand_placed(B, T3, NC)
    for buf, a in ((st.strong, strong), (st.strong_ema, strong_ema), (st.weak, weak), (st.weak_ema, weak_ema), (st.target, tgt)):
        buf.copy_(torch.tensor(a))
    _mt_loss_call(st, st.wlo, st.whi, st.slo, st.shi)
    m = _assert_loss_outputs(st, (0, 3, 1, 4), f"hand-placed nclass {NC}")
    assert m["cons_weight"] == pytest.approx(ref_cpu.consistency_weight(0, 150), rel=1e-6)


# ---- b / e. the three forms of the loss ---------------------------------------------------------------------------------------------
def _routes(B, T, groups, steer_s, steer_t, supervised=False, nclass=10, full_step=False, **kw):
    """One batch through the three forms of the loss on ONE MeanTeacherStep (the step state is not advanced in between):
      1  sed_mt_loss + sed_crnn_backward                      (k_mt_loss, k_heads_bwd with the gradients handed in)
      2  sed_mt_loss_backward                                 (the loss inside k_heads_bwd)
      3a sed_mt_step_backward under debug bit 24              (deferred heads, separate kernels)
      3b sed_mt_step_backward                                 (the loss inside the backward recurrence, csrc/hfuse.h, where it fuses)
    -> per route a dict of clones, and the step.
    What the comparison of the routes does NOT cover: 3b hands out no d_strong / d_weak (asking for them turns the fusion off),
    so only its posteriors and parameter gradients are compared; and in the supervised case strong_ema IS strong, so the
    posteriors are not cleared between the routes - a route that left them unwritten would go unnoticed there (with a teacher
    they are zeroed in front of 3a and 3b)."""
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.train import MeanTeacherStep
    l = _lib.lib()
    wlo, whi, slo, shi = groups
    wm = slice(wlo, whi) if whi > wlo else None
    sm = slice(slo, shi) if shi > slo else None
    student, ps = gu.make_model(0, dropout=0.5, nclass=nclass, **kw)
    gu.steer_model(student, ps, steer_s)
    student.train()
    teacher = None
    if not supervised:
        teacher, pt = gu.make_model(1, dropout=0.5, nclass=nclass, **kw)
        gu.steer_model(teacher, pt, steer_t)
        teacher.train()
    st = MeanTeacherStep(student, teacher, B, T, 150, wm, sm, seed=99, use_graph=False)
    assert (st.wlo, st.whi, st.slo, st.shi) == ((wlo, whi) if wm else (0, 0)) + ((slo, shi) if sm else (0, 0))
    g4 = (st.wlo, st.whi, st.slo, st.shi)
    tgt = _target01(7, B, T // 8, nclass)
    st.load_batch(synth.make_input(60, B, T).cuda(), synth.make_input(70, B, T).cuda(), tgt.cuda())
    if teacher is not None:
        st._forward(st.teacher, st.x_ema, st.ctx_t, st._seed_t, st.strong_ema, st.weak_ema)
    out = {}

    def snap(name, with_d):
        torch.cuda.synchronize()
        out[name] = dict(grads=st.grads.clone(), strong=st.strong.clone(), weak=st.weak.clone(), meters=dict(st.meters()),
                         d_strong=st.d_strong.clone() if with_d else None, d_weak=st.d_weak.clone() if with_d else None)

    def clear():
        st.grads.zero_(); st.d_strong.zero_(); st.d_weak.zero_(); st.losses[:8].zero_()

    # 1
    st._forward(st.student, st.x, st.ctx_s, st._seed_s, st.strong, st.weak)
    _mt_loss_call(st, *g4)
    _assert_loss_outputs(st, g4, f"groups {groups} sed_mt_loss")
    st._backward(3)
    snap("1", True)
    # 2
    clear()
    _lib.check(l.sed_mt_loss_backward(C.byref(st.dims), _lib.ptr(st.student._flat), _lib.ptr(st.x), st._seed_s,
                                      _lib.ptr(st.ctx_s), st.ctx_bytes, _lib.ptr(st.strong_ema), _lib.ptr(st.weak_ema),
                                      _lib.ptr(st.target), *g4, _lib.ptr(st.state), 0,
                                      _lib.ptr(st.losses), _lib.ptr(st.d_strong), _lib.ptr(st.d_weak), _lib.ptr(st.grads),
                                      _lib.ptr(st.ws), st.ws_bytes, 3, _lib.stream_ptr()), "sed_mt_loss_backward")
    snap("2", True)
    # 3a, 3b
    for name, debug, with_d in (("3a", SEPARATE_HEADS, True), ("3b", 0, False)):
        clear()
        if teacher is not None:                 # (supervised: strong_ema IS strong, which the call itself writes)
            st.strong.zero_(); st.weak.zero_()
        old = l.sed_debug_set(debug)
        try:
            st._forward(st.student, st.x, st.ctx_s, st._seed_s, None, None)
            _lib.check(l.sed_mt_step_backward(C.byref(st.dims), _lib.ptr(st.student._flat), _lib.ptr(st.x), st._seed_s,
                                              _lib.ptr(st.ctx_s), st.ctx_bytes, _lib.ptr(st.strong), _lib.ptr(st.weak),
                                              _lib.ptr(st.strong_ema), _lib.ptr(st.weak_ema), _lib.ptr(st.target), *g4,
                                              _lib.ptr(st.state), 0, _lib.ptr(st.losses),
                                              _lib.ptr(st.d_strong) if with_d else None, _lib.ptr(st.d_weak) if with_d else None,
                                              _lib.ptr(st.grads), _lib.ptr(st.ws), st.ws_bytes, 3, _lib.stream_ptr()),
                       "sed_mt_step_backward")
            snap(name, with_d)
        finally:
            l.sed_debug_set(old)
    if full_step:
        clear()
        st.run()
        torch.cuda.synchronize()
    return out, st, g4


def _assert_routes_agree(out, tag):
    a = out["1"]
    assert torch.isfinite(a["grads"]).all() and float(a["grads"].abs().max()) > 0, tag
    for name in ("2", "3a", "3b"):
        b = out[name]
        for k in ("strong", "weak", "grads", "d_strong", "d_weak"):
            if b[k] is not None:
                assert torch.equal(a[k], b[k]), (tag, name, k, float((a[k] - b[k]).abs().max()))
        for k, v in a["meters"].items():
            assert np.isfinite(b["meters"][k]), (tag, name, k)
            assert b["meters"][k] == pytest.approx(v, rel=2e-6, abs=1e-9), (tag, name, k)


GROUPS = [(4, (0, 0, 0, 0), False), (4, (0, 2, 0, 0), False), (4, (0, 0, 2, 4), False), (4, (0, 4, 0, 4), False),
          (4, (0, 3, 1, 4), False), (1, (0, 1, 0, 1), False), (4, (0, 0, 2, 4), True)]
GROUP_IDS = ["none", "weak-only", "strong-only", "all-in-both", "overlapping", "B1", "supervised-strong-only"]


@pytest.mark.parametrize("B,groups,supervised", GROUPS, ids=GROUP_IDS)
def test_label_group_edges_in_the_three_forms_of_the_loss(B, groups, supervised):
    """No labelled row at all, one group empty (with a teacher: slo == shi), every row in both groups, overlapping groups, B = 1;
    supervised with strong labels only.  The student sits on the ladder (exact 0 / 1 posteriors), the teacher is confident.
    sed_mt_loss holds against the float64 statement (an empty group's meters exactly 0.0; without labels the gradient is the
    consistency term alone), and the other forms are bit-identical to it in the gradients and the posteriors."""
    T = 136
    out, st, g4 = _routes(B, T, groups, "ladder", "confident", supervised=supervised)
    _assert_routes_agree(out, f"groups {groups}")
    if groups == (0, 0, 0, 0):
        s, se = out["1"]["strong"].cpu().double().numpy(), st.strong_ema.cpu().double().numpy()
        cw = out["1"]["meters"]["cons_weight"]
        np.testing.assert_allclose(out["1"]["d_strong"].cpu().numpy(), cw * 2.0 * (s - se) / s.size, rtol=1e-5, atol=1e-30)
        assert out["1"]["meters"]["loss"] == pytest.approx(out["1"]["meters"]["cons_strong"] + out["1"]["meters"]["cons_weak"], rel=1e-6)
    if supervised:
        assert out["1"]["meters"]["cons_strong"] == 0.0 and out["1"]["meters"]["cons_weak"] == 0.0


@pytest.mark.parametrize("B,T", [(3, 136), (2, 1040)])
@pytest.mark.parametrize("steering", ["ladder", "confident"])
def test_one_fused_step_with_student_and_teacher_steered(steering, B, T):
    """Both models in the same regime: the three forms bit-identical, then one whole step (forwards, loss, backward, Adam, EMA):
    its meters against the float64 statement on the posteriors the step stored, check_health(), finite parameters."""
    wm, sm = _groups_for(B)
    groups = (wm.start, wm.stop, sm.start, sm.stop)
    out, st, g4 = _routes(B, T, groups, steering, steering, full_step=True)
    _assert_routes_agree(out, f"{steering} ({B}, {T})")
    st.check_health()
    m = st.meters()
    want, _, _ = heads_np.mt_loss(*(t.cpu().numpy() for t in (st.strong, st.weak, st.strong_ema, st.weak_ema, st.target)), *g4,
                                  m["cons_weight"])
    for k, v in zip(heads_np.METERS[:7], want[:7]):
        assert m[k] == pytest.approx(v, rel=2e-5, abs=1e-9), (k, m[k], v)
    assert torch.isfinite(st.grads).all()
    assert torch.isfinite(st.student._flat).all() and torch.isfinite(st.teacher._flat).all()
    assert torch.isfinite(st.exp_avg).all() and torch.isfinite(st.exp_avg_sq).all()
    assert st.read_state().global_step == 1


# ---- c. heads forward on the kernel's own GRU output ------------------------------------------------------------------------------------
def _tail_metric(p, p64):
    """The smallest r with |p - p64| <= r min(p64, 1 - p64) + 2^-24 [p64 >= 0.5] + 1e-37 on every element (0 if none needs one);
    where the float64 tail itself is 0 no r helps: those elements must hold the absolute terms alone."""
    p, p64 = np.asarray(p, dtype=np.float64), np.asarray(p64, dtype=np.float64)
    tail = np.minimum(p64, 1.0 - p64)
    excess = np.abs(p - p64) - U24 * (p64 >= 0.5) - 1e-37
    assert (excess[tail == 0] <= 0).all(), "off where the float64 posterior is exactly 0 or 1"
    live = tail > 0
    return float(np.maximum(excess[live] / tail[live], 0.0).max())


# The ladder runs in train mode (dropout 0.5) and in eval mode on every shape.  The confident steering runs where its guard
# min(p, 1 - p) >= 1e-4 can hold.  Dropout doubles the kept activations: at (2, 16) the smallest tail stays at 8e-5 .. 2.2e-3
# (above 1e-4 at 27 of 30 seed pairs), so that shape runs with dropout 0.5; at (3, 136) it is 1.7e-5 at best and at (2, 1040)
# 2.6e-6, so those run in eval mode and in train mode without dropout.  The wide model, whose heads sum over 512 features, is at
# 3e-5 in eval mode and at most 7.5e-6 in train mode at every seed: no confident case there.
# (tests/test_heads_regimes_cpu.py::test_where_the_confident_steering_cannot_keep_its_tail_guard asserts these.)
FWD_CASES = [(B, T, kw, "ladder", 10, mode) for (B, T, kw) in SHAPES for mode in ("train", "eval")]
FWD_CASES += [(3, 136, {}, "ladder", nc, mode) for nc in (16, 1) for mode in ("train", "eval")]      # the ABI's limits on nclass
FWD_CASES += [(B, T, {}, "confident", 10, "eval") for (B, T) in ((2, 16), (3, 136), (2, 1040))]
FWD_CASES += [(B, T, {}, "confident", 10, "train0") for (B, T) in CONFIDENT_TRAIN_SHAPES]
FWD_CASES += [(B, T, {}, "confident", 10, "train") for (B, T) in CONFIDENT_DROPOUT_SHAPES]
FWD_IDS = [f"{'wide-' if kw else ''}{B}x{T}-{steering}-nc{nc}-{mode}" for (B, T, kw, steering, nc, mode) in FWD_CASES]


@pytest.mark.parametrize("B,T,kw,steering,nclass,mode", FWD_CASES, ids=FWD_IDS)
def test_heads_forward_against_the_float64_statement_on_the_kernels_own_gru_output(B, T, kw, steering, nclass, mode):
    """strong, the attention and its clamp mask, den and weak of a forward against tests/heads_np.heads_forward evaluated on the
    GRU output that forward itself stored (ctx 'gru1') and the Philox mask of its dropout."""
    H, T3, p = kw.get("H", 64), T // 8, 0.5 if mode == "train" else 0.0
    train = mode == "train"
    model, params = gu.make_model(0, dropout=p, nclass=nclass, **kw)
    params = gu.steer_model(model, params, steering)
    model.train(mode != "eval")
    x = synth.make_input(_x_seed(steering, B, T, mode), B, T).cuda()
    with torch.no_grad():
        s, w = model(x, seed=gu.seed_tensor(DROP_SEED) if train else None)
    torch.cuda.synchronize()
    att = model.last_attention().cpu().numpy()
    gru = model.ctx_view("gru1").view(B, T3, 2 * H).cpu().numpy()
    logits = model.ctx_view("logits_s").view(B, T3, nclass).cpu().numpy()
    den = model.ctx_view("den").view(B, nclass).cpu().numpy()
    s, w = s.cpu().numpy(), w.cpu().numpy()
    mask = philox.dropout_mask_flat(DROP_SEED, 8, (B, T3, 2 * H), p) if train else np.float32(1.0)
    heads = [params[n].numpy() for n in gu.HEAD_NAMES]
    s64, raw, att64, den64, w64 = heads_np.heads_forward(gru, mask, *heads)
    _guards(raw, s64, steering)
    tag = f"{steering} nclass {nclass} ({B}, {T}){' wide' if kw else ''} {mode}"
    for a in (s, w, att, den, logits):
        assert np.isfinite(a).all(), tag
    # the attention: the same elements clamped, values within the suite's posterior tolerance
    assert ((att <= np.float32(1e-7)) == (raw < heads_np.ATT_MIN)).all(), tag
    assert (att >= np.float32(1e-7)).all() and (att <= 1).all()
    assert np.abs(att - att64).max() < tp.POST_TOL, tag
    # den and weak: sums of positive terms - against the statement on the kernel's own strong and attention, any order
    den_k, weak_k = heads_np.pool(s, att)
    tol = (2 * T3 + 4) * U24
    assert (np.abs(den - den_k) <= tol * den_k + 1e-37).all(), (tag, float((np.abs(den - den_k) / den_k).max()))
    assert (np.abs(w - weak_k) <= tol * weak_k + 1e-37).all(), (tag, float(np.abs(w - weak_k).max()))
    assert np.abs(w - w64).max() < tp.POST_TOL, tag
    # strong: absolutely, and relative to the tail.  r = 4 x the same metric of the reference's own arithmetic (torch float32
    # F.linear + sigmoid of the same h on the CPU): v_exp and v_rcp at ~1 ulp each plus the z log2(e) rounding that grows with |z|
    assert np.abs(s - s64).max() < tp.POST_TOL, tag
    x32 = torch.tensor(gru) * torch.tensor(np.broadcast_to(mask, gru.shape).copy())
    ref32 = torch.sigmoid(F.linear(x32, params["dense.weight"], params["dense.bias"])).numpy()
    r_ref, r_hip = _tail_metric(ref32, s64), _tail_metric(s, s64)
    print(f"[heads regimes] {tag}: tail-relative error of strong: reference fp32 {r_ref:.3e}, kernel {r_hip:.3e} (bound 4 x reference); "
          f"clamped {float((raw < heads_np.ATT_MIN).mean()):.3f}, strong {s64.min():.2e} .. 1 - {1 - s64.max():.2e}")
    assert r_hip <= 4 * r_ref, (tag, r_hip, r_ref)
    if steering == "ladder" and nclass == 10:
        assert (s[..., 0] == 0.0).all() and (s[..., 8:] == 1.0).all(), tag
        assert (w[:, 0] == 0.0).all() and (w[:, 8:] == 1.0).all(), tag
        assert ((raw < heads_np.ATT_MIN).all(axis=(0, 1)) == np.array([False] * 5 + [True] * 5)).all(), tag


# ---- d. backward, end to end, through the autograd module path ------------------------------------------------------------------
def _typ_err(g, ref):
    """err / typical magnitude, the metric of test_gpu_parity._check_grads."""
    ref = ref.double()
    return float((g.double() - ref).abs().max()) / (float(ref.norm()) / np.sqrt(ref.numel()) + 1e-30)


@pytest.mark.parametrize("B,T,kw", SHAPES, ids=SHAPE_IDS)
def test_backward_on_the_ladder_against_the_float32_oracle(B, T, kw):
    """Exact saturation, end to end.  The float32 oracle is the reference here: 1 - 9e-14 is 1 in float32 and not in float64, whose
    loss and gradient differ by construction."""
    tgt = (_target01(5, B, T // 8, 10),) + _groups_for(B)
    hip, orc = tp._fwd_bwd_both(B, T, 0.5, DROP_SEED, steer="ladder", target=tgt, x_seed=_x_seed("ladder", B, T, "train"), **kw)
    assert (hip[0][..., 0] == 0).all() and (hip[0][..., 8:] == 1).all()
    assert float((hip[0] - orc[0]).abs().max()) < tp.POST_TOL and float((hip[1] - orc[1]).abs().max()) < tp.POST_TOL
    assert np.isfinite(hip[2]) and hip[2] == pytest.approx(orc[2], rel=1e-5)
    for n, g in hip[3].items():
        assert torch.isfinite(g).all(), n
    worst = tp._check_grads(hip[3], orc[3])
    print(f"[heads regimes] ladder ({B}, {T}){' wide' if kw else ''} backward vs float32 oracle: worst err/typ {worst:.3e}")


BWD_CONFIDENT = [(B, T, 0.5) for (B, T) in CONFIDENT_DROPOUT_SHAPES] + [(B, T, 0.0) for (B, T) in CONFIDENT_TRAIN_SHAPES]


@pytest.mark.parametrize("B,T,p", BWD_CONFIDENT, ids=[f"{B}x{T}-p{p}" for (B, T, p) in BWD_CONFIDENT])
def test_backward_in_the_confident_regime_against_the_float64_oracle(B, T, p):
    """No cliff, so float64 is the reference.  A tensor's bound is the larger of _check_grads's and 4 x e_ref, e_ref the float32
    oracle's own error against the float64 oracle on the same inputs in the same err / typical metric, computed here
    (profiles/heads_regimes.md has its size per case).  Train mode, with dropout 0.5 where the guards hold with it ((2, 16)) and
    without dropout on the three H = 64 shapes (FWD_CASES says why)."""
    mode = "train" if p > 0 else "train0"
    tgt = (_target01(5, B, T // 8, 10),) + _groups_for(B)
    xs = _x_seed("confident", B, T, mode)
    hip, o32, o64 = tp._fwd_bwd_both(B, T, p, DROP_SEED if p > 0 else None, steer="confident", target=tgt, x_seed=xs,
                                     oracle_dtypes=(torch.float32, torch.float64))
    s64 = o64[0].numpy()
    p64 = {k: v.double() for k, v in gu.steer_heads(synth.make_params(0), "confident").items()}
    masks = gu.oracle_masks(DROP_SEED, B, T, p)
    masks = None if masks is None else {k: v.double() for k, v in masks.items()}
    with torch.no_grad():
        gru64 = ref_cpu.crnn_forward(p64, synth.make_input(xs, B, T).double(), True, ref_cpu.new_bn_state(dtype=torch.float64), masks,
                                     return_intermediates=True)[2]["gru1"]
        if masks is not None:
            gru64 = gru64 * masks["drop_rnn"]
        raw64 = torch.softmax(F.linear(gru64, p64["dense_softmax.weight"], p64["dense_softmax.bias"]), dim=-1).numpy()
    _guards(raw64, s64, "confident")
    assert float((hip[0].double() - o64[0]).abs().max()) < tp.POST_TOL and float((hip[1].double() - o64[1]).abs().max()) < tp.POST_TOL
    # the loss: 1e-5 as everywhere, or 4 x the float32 oracle's own distance (a posterior of 2e-4 moves its logarithm by 2.5e-3 per 5e-7)
    assert hip[2] == pytest.approx(o64[2], rel=max(1e-5, 4 * abs(o32[2] - o64[2]) / abs(o64[2])))
    print(f"[heads regimes] confident ({B}, {T}) p {p} loss: float64 {o64[2]:.9f} float32 oracle {o32[2]:.9f} kernel {hip[2]:.9f}")
    e_ref = {n: _typ_err(o32[3][n], o64[3][n]) for n in o64[3]}
    e_hip = {n: _typ_err(hip[3][n], o64[3][n]) for n in o64[3]}
    for pre in ("cnn.", "rnn.", "dense.", "dense_softmax."):
        ns = [n for n in e_ref if n.startswith(pre) and not (".conv" in n and n.endswith("bias"))]
        print(f"[heads regimes] confident ({B}, {T}) p {p} {pre:15s} e_ref max {max(e_ref[n] for n in ns):.3e}  kernel max {max(e_hip[n] for n in ns):.3e}")
    tp._check_grads(hip[3], {n: g.float() for n, g in o64[3].items()}, floor={n: 4 * e for n, e in e_ref.items()})


_ATT = {}


def _att_case(B, T):
    """Ladder, dropout 0: the weights of loss = sum ws strong + sum ww weak + sum wa att and its float64 oracle gradients."""
    if (B, T) not in _ATT:
        rs = np.random.RandomState(9)
        ws, ww, wa = (torch.tensor(rs.standard_normal(shp), dtype=torch.float32) for shp in ((B, T // 8, 10), (B, 10), (B, T // 8, 10)))
        params = gu.steer_heads(synth.make_params(0), "ladder")
        po = {k: v.double().requires_grad_(True) for k, v in params.items()}
        so, wo, inter = ref_cpu.crnn_forward(po, synth.make_input(40, B, T).double(), True, ref_cpu.new_bn_state(dtype=torch.float64), None,
                                             return_intermediates=True)
        raw = torch.softmax(F.linear(inter["gru1"], po["dense_softmax.weight"], po["dense_softmax.bias"]), dim=-1)
        att = torch.clamp(raw, min=heads_np.ATT_MIN, max=1)
        lo = (so * ws.double()).sum() + (wo * ww.double()).sum() + (att * wa.double()).sum()
        names = ["dense_softmax.weight", "dense_softmax.bias"]
        _ATT[(B, T)] = dict(ws=ws, ww=ww, wa=wa, raw=raw.detach().numpy(), att=att.detach(),
                            go=dict(zip(names, torch.autograd.grad(lo, [po[n] for n in names]))))
    return _ATT[(B, T)]


def test_backward_att_on_the_ladder():
    """sed_crnn_backward_att with a random attention gradient where half the classes are clamped in every frame: the
    dense_softmax gradients against float64 autograd, and d_att on the classes whose pass mask is 0 everywhere changes no bit."""
    B, T = 3, 136
    c = _att_case(B, T)
    _guards(c["raw"], None, "ladder")
    dead = (c["raw"] < heads_np.ATT_MIN).all(axis=(0, 1))
    assert (dead == np.array([False] * 5 + [True] * 5)).all()
    ws, ww, wa = c["ws"].cuda(), c["ww"].cuda(), c["wa"].cuda()
    wa_dead = wa * torch.tensor(dead, dtype=torch.float32).cuda()

    def grads(wa_used):
        model, params = gu.make_model(0, dropout=0.0)
        gu.steer_model(model, params, "ladder")
        model.train()
        s, w, att = model(synth.make_input(40, B, T).cuda(), return_attention=True)
        ((s * ws).sum() + (w * ww).sum() + (att * wa_used).sum()).backward()
        torch.cuda.synchronize()
        return gu.grads_dict(model), att.detach().cpu()

    g, att = grads(wa)
    assert float((att.double() - c["att"]).abs().max()) < tp.POST_TOL
    assert ((att.numpy() <= np.float32(1e-7)) == (c["raw"] < heads_np.ATT_MIN)).all()
    for n in g:
        assert torch.isfinite(g[n]).all(), n
    worst = tp._check_grads({n: g[n] for n in c["go"]}, {n: v.float() for n, v in c["go"].items()})
    print(f"[heads regimes] backward_att on the ladder, dense_softmax.* vs float64: worst err/typ {worst:.3e}")
    g_dead, _ = grads(wa_dead)
    g_none, _ = grads(torch.zeros_like(wa))
    for n in g_none:
        assert g_dead[n].numpy().tobytes() == g_none[n].numpy().tobytes(), n
    assert any(g[n].numpy().tobytes() != g_none[n].numpy().tobytes() for n in g)

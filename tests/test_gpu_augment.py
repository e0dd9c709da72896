"""-m gpu tests of the train-time batch augmentation: sed_batch_augment against the numpy statement of its definitions
(tests/augment_np.py), bit for bit; its argument checks; soft (mixed) targets through the loss kernels; the resident
front-end with a policy against the serial order, against host feeding and against the un-augmented run."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import features_np, ref_cpu, synth
from tests import augment_np
from tests import gpu_util as gu

pytestmark = pytest.mark.gpu
PHI = 0x9E3779B97F4A7C15
ONE = int(np.float32(1.0).view(np.int32))


def _bits(v):
    return int(np.float32(v).view(np.int32))


def _same_bits(got, want):
    """Bitwise equality (torch.equal on the int32 views, so NaN payloads and signed zeros count too)."""
    return torch.equal(got.detach().cpu().contiguous().view(torch.int32), torch.from_numpy(np.ascontiguousarray(want)).view(torch.int32))


def _poisoned(like):
    """An output buffer of the shape of ``like`` pre-filled with 0xFF bytes (NaN)."""
    return torch.full(like.shape, -1, dtype=torch.int32, device="cuda").view(torch.float32)


def _launch(x, xe, g, table, out_x, out_xe, out_g, B=None, T=None, M=None, T3=None, NC=None):
    from dcase2019_task4_amd import _lib
    B = x.shape[0] if B is None else B
    T = x.shape[-2] if T is None else T
    M = x.shape[-1] if M is None else M
    T3 = (g.shape[1] if g is not None else 0) if T3 is None else T3
    NC = (g.shape[2] if g is not None else 0) if NC is None else NC
    _lib.check(_lib.lib().sed_batch_augment(_lib.ptr(x), _lib.ptr(xe), _lib.ptr(g), _lib.ptr(table), B, T, M, T3, NC,
                                            _lib.ptr(out_x), _lib.ptr(out_xe), _lib.ptr(out_g), _lib.stream_ptr()),
               "sed_batch_augment")
    torch.cuda.synchronize()


def _run(x, xe, g, table):
    """The kernel through the C-ABI on NaN-filled outputs."""
    tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).cuda()
    outs = [None if t is None else _poisoned(t) for t in (x, xe, g)]
    _launch(x, xe, g, tab, *outs)
    return outs


def _case(B, T, M, T3, NC, seed, nan_clip):
    rs = np.random.RandomState(seed)
    X = rs.standard_normal((B, T, M)).astype(np.float32)
    Xe = (X + np.abs(rs.standard_normal((B, T, M)) * 0.5)).astype(np.float32)
    G = rs.uniform(0, 1, (B, T3, NC)).astype(np.float32)
    for A in (X, Xe, G):
        A[nan_clip] = np.nan
    return X, Xe, G


def _table5(T, M):
    """B = 5; clip 4 holds NaN."""
    return np.array([
        [0, ONE, 0, 0, 0, 0, 0, 0],                                   # identity
        [2, _bits(0.3), 5, 1, M - 3, 9, -1, 3],                       # everything at once: a partner with a shift of its own,
                                                                      # lambda inside (0, 1), both masks overrunning an edge
        [2, _bits(0.5), -(T + 3), -4, 0, 2, T - 2, 2],                # self-partner; negative shifts beyond n; masks touching both edges
        [4, ONE, 3 * T + 1, 7, 3, 0, 2, -4],                          # lambda = 1 with a NaN partner (must not leak); zero / negative widths
        [4, _bits(0.25), 1, 1, 0, 0, 0, 0],                           # NaN clip, self-partner, rolled: copied bit for bit
    ], dtype=np.int32)


def _table3(T, M):
    """B = 3; clip 2 holds NaN."""
    return np.array([
        [1, _bits(0.3), 2, 1, 0, 0, 0, 0],                            # a plain mix, lambda inside (0, 1), the partner shifted the other way
        [0, _bits(0.9), -13, -3, -1, 3, T - 2, 5],                    # negative shift beyond T, masks overrunning both kinds of edge
        [0, ONE, 2 ** 31 - 1, -2 ** 31, M, 4, T, 4],                  # extreme shifts, lambda = 1 (copy of a NaN clip), masks wholly outside
    ], dtype=np.int32)


CASES = {"5x24x64": ((5, 24, 64, 3, 10), _table5, 4), "3x9x7": ((3, 9, 7, 2, 3), _table3, 2)}


@pytest.mark.parametrize("variant", ["all", "no_x_ema", "no_target", "x_only", "unaligned_base", "b1tm"])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_vs_numpy_statement_bit_exact(case, variant):
    (B, T, M, T3, NC), table_fn, nan_clip = CASES[case]
    X, Xe, G = _case(B, T, M, T3, NC, 17 + B, nan_clip)
    table = table_fn(T, M)
    if variant in ("no_x_ema", "x_only"):
        Xe = None
    if variant in ("no_target", "x_only"):
        G = None
    wx, wxe, wg = augment_np.augment(X, Xe, G, table)
    if variant == "unaligned_base":
        # bases 4 bytes past a 16-byte boundary: the scalar path also for M % 4 == 0
        dev = [None if a is None else torch.cat([torch.zeros(1), torch.from_numpy(a).reshape(-1)]).cuda()[1:].view(a.shape)
               for a in (X, Xe, G)]
        assert dev[0].data_ptr() % 16 == 4
    elif variant == "b1tm":
        dev = [torch.from_numpy(X).cuda().view(B, 1, T, M), torch.from_numpy(Xe).cuda().view(B, 1, T, M), torch.from_numpy(G).cuda()]
        wx, wxe = wx.reshape(B, 1, T, M), wxe.reshape(B, 1, T, M)
    else:
        dev = [None if a is None else torch.from_numpy(a).cuda() for a in (X, Xe, G)]
    ox, oxe, og = _run(*dev, table)
    assert _same_bits(ox, wx)
    assert (oxe is None) == (Xe is None) and (og is None) == (G is None)
    if Xe is not None:
        assert _same_bits(oxe, wxe)
    if G is not None:
        assert _same_bits(og, wg)
    # the NaN clip reached only its own output rows; a masked element is +0.0
    clean = [b for b in range(B) if b != nan_clip]
    assert torch.isfinite(ox.reshape(B, T, M)[clean]).all() and torch.isnan(ox.reshape(B, T, M)[nan_clip]).any()
    if case == "5x24x64":
        assert _same_bits(ox.reshape(B, T, M)[1, :2], np.zeros((2, M), np.float32))
        assert _same_bits(ox.reshape(B, T, M)[1, :, M - 3:], np.zeros((T, 3), np.float32))


def test_augment_batch_equals_the_direct_call_and_validates_host_tables():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.augment import augment_batch
    (B, T, M, T3, NC), table_fn, nan_clip = CASES["5x24x64"]
    X, Xe, G = _case(B, T, M, T3, NC, 3, nan_clip)
    table = table_fn(T, M)
    want = augment_np.augment(X, Xe, G, table)
    x, xe, g = (torch.from_numpy(a).cuda() for a in (X, Xe, G))
    for tab in (table, torch.from_numpy(table).cuda()):
        got = augment_batch(x.view(B, 1, T, M), xe.view(B, 1, T, M), g, tab)
        assert got[0].shape == (B, 1, T, M)
        assert all(_same_bits(a, w.reshape(a.shape)) for a, w in zip(got, want))
    gx, gxe, gg = augment_batch(x, None, None, table)
    assert gxe is None and gg is None and _same_bits(gx, want[0])
    bad = table.copy()
    bad[1, 0] = B
    for t in (bad, table.astype(np.int64), table[:4], np.stack([table, table])):
        with pytest.raises(_lib.SedError):
            augment_batch(x, xe, g, t)


def test_identity_table_returns_the_inputs():
    from dcase2019_task4_amd.augment import identity_table
    for (B, T, M, T3, NC), _, nan_clip in CASES.values():
        X, Xe, G = _case(B, T, M, T3, NC, 5, nan_clip)
        dev = [torch.from_numpy(a).cuda() for a in (X, Xe, G)]
        outs = _run(*dev, identity_table(B))
        for o, a in zip(outs, (X, Xe, G)):
            assert _same_bits(o, a)


def test_argument_checks_on_real_buffers():
    """An output aliasing an input, a partial pair and non-positive sizes return SED_ERR_BAD_ARG before anything is launched:
    the NaN-filled outputs stay NaN."""
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.augment import identity_table
    B, T, M, T3, NC = 3, 9, 8, 2, 3
    X, Xe, G = _case(B, T, M, T3, NC, 1, 2)
    x, xe, g = (torch.from_numpy(np.nan_to_num(a)).cuda() for a in (X, Xe, G))
    tab = torch.from_numpy(identity_table(B)).cuda()
    ox, oxe, og = _poisoned(x), _poisoned(xe), _poisoned(g)
    _launch(x, xe, g, tab, ox, oxe, og)                       # the good call, for contrast
    assert torch.equal(ox, x) and torch.equal(oxe, xe) and torch.equal(og, g)
    big = torch.zeros(2 * x.numel(), device="cuda")
    half = big[x.numel() // 2:x.numel() // 2 + x.numel()].view(B, T, M)       # overlaps big[:numel] by half
    bad_calls = {
        "out_x is x": lambda: _launch(x, xe, g, tab, x, oxe, og),
        "out_x is x_ema": lambda: _launch(x, xe, g, tab, xe, oxe, og),
        "out_x_ema is x": lambda: _launch(x, xe, g, tab, ox, x, og),
        "out_target is target": lambda: _launch(x, xe, g, tab, ox, oxe, g),
        "partial overlap": lambda: _launch(big[:x.numel()].view(B, T, M), None, None, tab, half, None, None),
        "outputs overlap": lambda: _launch(x, xe, None, tab, big[:x.numel()].view(B, T, M), half, None),
        "x_ema without out_x_ema": lambda: _launch(x, xe, g, tab, ox, None, og),
        "out_x_ema without x_ema": lambda: _launch(x, None, g, tab, ox, oxe, og),
        "target without out_target": lambda: _launch(x, xe, g, tab, ox, oxe, None, T3=T3, NC=NC),
        "out_target without target": lambda: _launch(x, xe, None, tab, ox, oxe, og, T3=T3, NC=NC),
        "no table": lambda: _launch(x, xe, g, None, ox, oxe, og),
        "B = 0": lambda: _launch(x, xe, g, tab, ox, oxe, og, B=0),
        "T = 0": lambda: _launch(x, xe, g, tab, ox, oxe, og, T=0),
        "M = -1": lambda: _launch(x, xe, g, tab, ox, oxe, og, M=-1),
        "T3 = 0": lambda: _launch(x, xe, g, tab, ox, oxe, og, T3=0),
        "NC = 0": lambda: _launch(x, xe, g, tab, ox, oxe, og, NC=0),
    }
    keep = (x.clone(), xe.clone(), g.clone())
    for name, call in bad_calls.items():
        ox, oxe, og = _poisoned(x), _poisoned(xe), _poisoned(g)
        with pytest.raises(_lib.SedError, match="status -?[0-9]+"):
            call()
        torch.cuda.synchronize()
        assert torch.isnan(ox).all() and torch.isnan(oxe).all() and torch.isnan(og).all(), name
        assert torch.equal(x, keep[0]) and torch.equal(xe, keep[1]) and torch.equal(g, keep[2]), name
        assert not big.any(), name


# ---- soft targets through the loss -----------------------------------------------------------------------------------------
def _mixed_target(B, T3):
    """synth.make_target's [weak | unlabelled | strong] batch mixed within its slices by the kernel: lambda in (0, 1), labelled
    rows only in the labelled slices (and the unlabelled -1 rows only with each other)."""
    from dcase2019_task4_amd.augment import augment_batch
    tgt, wm, sm = synth.make_target(3, B, T3)
    nw = B // 4
    lam = np.random.RandomState(8).uniform(0.15, 0.85, B).astype(np.float32)
    table = np.zeros((B, 8), np.int32)
    for b in range(B):
        lo, hi = (0, nw) if b < nw else ((B - nw, B) if b >= B - nw else (nw, B - nw))
        table[b] = [lo + (b - lo + 1) % (hi - lo), _bits(lam[b]), 0, (b % 3) - 1, 0, 0, 0, 0]
    x = torch.zeros(B, 8, 4, device="cuda")
    _, _, mixed = augment_batch(x, None, tgt.cuda(), table)
    want = augment_np.augment(np.zeros((B, 8, 4), np.float32), None, tgt.numpy(), table)[2]
    assert _same_bits(mixed, want)
    lab = torch.cat([mixed[wm], mixed[sm]]).cpu()
    assert ((lab > 0) & (lab < 1)).any() and lab.min() >= 0 and lab.max() <= 1          # soft, and still a probability
    assert (mixed[nw:B - nw].cpu() < 0).all()
    return mixed.cpu(), wm, sm


def test_mt_loss_kernel_vs_oracle_on_mixed_targets():
    """tests/test_gpu_parity.py::test_mt_loss_kernel_vs_oracle with a mixed (soft) target, its assertions and tolerances."""
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.train import MeanTeacherStep
    B, T = 8, 128
    student, _ = gu.make_model(0, dropout=0)
    teacher, _ = gu.make_model(1, dropout=0)
    tgt, wm, sm = _mixed_target(B, T // 8)
    st = MeanTeacherStep(student, teacher, B, T, 150, wm, sm, use_graph=False)
    rs = np.random.RandomState(5)
    for name in ("strong", "strong_ema"):
        getattr(st, name).copy_(torch.tensor(rs.uniform(0.02, 0.98, (B, T // 8, 10)), dtype=torch.float32))
    for name in ("weak", "weak_ema"):
        getattr(st, name).copy_(torch.tensor(rs.uniform(0.02, 0.98, (B, 10)), dtype=torch.float32))
    st.target.copy_(tgt)
    _lib.check(st.l.sed_mt_loss(C.byref(st.dims), _lib.ptr(st.strong), _lib.ptr(st.weak), _lib.ptr(st.strong_ema),
                                _lib.ptr(st.weak_ema), _lib.ptr(st.target), st.wlo, st.whi, st.slo, st.shi,
                                _lib.ptr(st.state), _lib.ptr(st.losses), _lib.ptr(st.d_strong), _lib.ptr(st.d_weak),
                                _lib.stream_ptr()), "sed_mt_loss")
    s = st.strong.cpu().requires_grad_(True)
    w = st.weak.cpu().requires_grad_(True)
    cw = ref_cpu.consistency_weight(0, 150)
    loss, meters = ref_cpu.mean_teacher_loss(s, w, st.strong_ema.cpu(), st.weak_ema.cpu(), tgt, wm, sm, cw)
    ds, dw = torch.autograd.grad(loss, [s, w])
    m = st.meters()
    for k in ("loss", "weak_class_loss", "strong_loss", "cons_strong", "cons_weak", "weak_ema_loss", "strong_ema_loss"):
        print(f"[soft loss] {k:16s} kernel {m[k]:.9g} oracle {float(meters[k]):.9g}")
        assert m[k] == pytest.approx(float(meters[k]), rel=2e-5, abs=1e-9), k
    assert m["cons_weight"] == pytest.approx(cw, rel=1e-6)
    np.testing.assert_allclose(st.d_strong.cpu().numpy(), ds.numpy(), rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(st.d_weak.cpu().numpy(), dw.numpy(), rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("T", [128, 216])
def test_fused_loss_backward_matches_loss_kernel_then_backward_on_mixed_targets(T):
    """tests/test_gpu_parity.py::test_fused_loss_backward_matches_loss_kernel_then_backward with a mixed (soft) target: the
    same equalities (T = 216 is that test's own shape, T = 128 the loss test's)."""
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.train import MeanTeacherStep
    B = 8
    student, _ = gu.make_model(0, dropout=0.5)
    teacher, _ = gu.make_model(1, dropout=0.5)
    student.train(); teacher.train()
    tgt, wm, sm = _mixed_target(B, T // 8)
    st = MeanTeacherStep(student, teacher, B, T, 150, wm, sm, seed=99, use_graph=False)
    st.load_batch(synth.make_input(60, B, T).cuda(), synth.make_input(70, B, T).cuda(), tgt.cuda())
    st._forward(st.teacher, st.x_ema, st.ctx_t, st._seed_t, st.strong_ema, st.weak_ema)
    st._forward(st.student, st.x, st.ctx_s, st._seed_s, st.strong, st.weak)
    # (a) separate kernels
    _lib.check(st.l.sed_mt_loss(C.byref(st.dims), _lib.ptr(st.strong), _lib.ptr(st.weak), _lib.ptr(st.strong_ema),
                                _lib.ptr(st.weak_ema), _lib.ptr(st.target), st.wlo, st.whi, st.slo, st.shi,
                                _lib.ptr(st.state), _lib.ptr(st.losses), _lib.ptr(st.d_strong), _lib.ptr(st.d_weak),
                                _lib.stream_ptr()), "sed_mt_loss")
    st._backward(3)
    torch.cuda.synchronize()
    ds_a, dw_a, g_a, m_a = st.d_strong.clone(), st.d_weak.clone(), st.grads.clone(), dict(st.meters())
    # (b) fused
    st.grads.zero_(); st.d_strong.zero_(); st.d_weak.zero_()
    _lib.check(st.l.sed_mt_loss_backward(C.byref(st.dims), _lib.ptr(st.student._flat), _lib.ptr(st.x), st._seed_s,
                                         _lib.ptr(st.ctx_s), st.ctx_bytes, _lib.ptr(st.strong_ema), _lib.ptr(st.weak_ema),
                                         _lib.ptr(st.target), st.wlo, st.whi, st.slo, st.shi, _lib.ptr(st.state), 0,
                                         _lib.ptr(st.losses), _lib.ptr(st.d_strong), _lib.ptr(st.d_weak), _lib.ptr(st.grads),
                                         _lib.ptr(st.ws), st.ws_bytes, 3, _lib.stream_ptr()), "sed_mt_loss_backward")
    torch.cuda.synchronize()
    assert torch.isfinite(st.grads).all() and st.grads.abs().max() > 0
    assert torch.equal(st.d_strong, ds_a) and torch.equal(st.d_weak, dw_a)
    assert torch.equal(st.grads, g_a)
    m_b = st.meters()
    for k, v in m_a.items():
        print(f"[soft fused] {k:16s} separate {v:.9g} fused {m_b[k]:.9g}")
        assert m_b[k] == pytest.approx(v, rel=2e-6, abs=1e-9), k


# ---- the resident front-end with a policy ------------------------------------------------------------------------------------
def _clips(lengths, seed=0, n_mels=64):
    rs = np.random.RandomState(seed)
    return [(np.abs(rs.standard_normal((n, n_mels))) * 3.0).astype(np.float32) for n in lengths]


def _policy():
    from dcase2019_task4_amd.augment import AugmentPolicy
    return AugmentPolicy(mixup_alpha=0.4, mixup_prob=0.8, shift_std=6.0, freq_mask_max=10, time_mask_max=60, seed=31)


_POOL = {}


def _train_set(augment, ragged):
    """The pool of tests/test_gpu_resident.py::_train_set (8 clips per batch, 3 steps per epoch, T = 628), rebuilt here; the
    host arrays and the scaler are computed once and shared."""
    from dcase2019_task4_amd.features import Scaler
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    T = 628
    sizes, bsz = (8, 12, 8), (2, 4, 2)
    if ragged not in _POOL:
        seed = 0 if ragged else 1
        rs_ = np.random.RandomState(seed)
        lengths = [int(rs_.randint(560, 700)) if ragged else T for _ in range(sum(sizes))]
        feats = _clips(lengths, 20 + seed)
        tgts = []
        for i in range(sum(sizes)):
            r = np.random.RandomState(300 + i)
            if i < sizes[0]:
                tgts.append(np.repeat((r.uniform(size=(1, 10)) < 0.3).astype(np.float32), T // 8, axis=0))
            elif i < sizes[0] + sizes[1]:
                tgts.append(-np.ones((T // 8, 10), np.float32))
            else:
                tgts.append((r.uniform(size=(T // 8, 10)) < 0.2).astype(np.float32))
        sc = Scaler()
        sc.calculate_scaler([features_np.transform_chain(f, T) for f in feats[:4]])
        _POOL[ragged] = feats, tgts, sc
    feats, tgts, sc = _POOL[ragged]
    return ResidentFeatureSet.from_arrays(feats, tgts, sizes, bsz, frames=T, scaler=sc, seed=5, augment=augment)


def _mt_step(rs, seed=99):
    from dcase2019_task4_amd.train import MeanTeacherStep
    student, _ = gu.make_model(0, dropout=0.5)
    teacher, _ = gu.make_model(1, dropout=0.5)
    student.train(); teacher.train()
    st = MeanTeacherStep(student, teacher, rs.batch, rs.frames, 100, rs.weak_mask, rs.strong_mask, seed=seed, use_graph=True)
    return st, student, teacher


def _front_end_run(rs, overlap=True, np_seed=2024, n=7):
    from dcase2019_task4_amd.resident import ResidentFrontEnd
    np.random.seed(np_seed)
    st, s, t = _mt_step(rs)
    fe = ResidentFrontEnd(st, rs, overlap=overlap)
    assert fe.overlap == overlap
    meters = []
    for _ in range(n):
        fe.run()
        meters.append(st.meters())
    torch.cuda.synchronize()
    assert st.steps_done == n and fe._epoch == 2 and fe._pos == 2
    tables = {e: t.copy() for e, t in fe.host_tables.items()}
    st.close()
    return s._flat.clone(), t._flat.clone(), meters, tables


_RUNS = {}


def _shared_run(kind):
    """Front-end runs several tests compare against, computed once: 7 steps over 3-step epochs, ragged pool, overlap on."""
    if kind not in _RUNS:
        aug = {"augmented": _policy, "plain": lambda: None}[kind]()
        _RUNS[kind] = _front_end_run(_train_set(aug, ragged=True))
    return _RUNS[kind]


def test_front_end_with_a_policy_one_batch_ahead_equals_serial_and_the_policy_is_live():
    """7 steps across two epoch boundaries with all three augmentations on: the in-graph gather + augment of batch k + 1 leaves
    student, teacher and meters bit-identical to the serial protocol; the student differs from the un-augmented run's."""
    serial = _front_end_run(_train_set(_policy(), ragged=True), overlap=False)
    ahead = _shared_run("augmented")
    assert torch.equal(serial[0], ahead[0]) and torch.equal(serial[1], ahead[1])
    assert serial[2] == ahead[2] and all(np.isfinite(m["loss"]) for m in ahead[2])
    plain = _shared_run("plain")
    assert not torch.equal(plain[0], ahead[0])
    assert all(np.array_equal(plain[3][e], ahead[3][e]) for e in plain[3])           # the same clips, differently augmented


def test_off_means_off():
    """A policy with everything off and no policy at all: bit-identical students and the same index tables."""
    from dcase2019_task4_amd.augment import AugmentPolicy
    off = _front_end_run(_train_set(AugmentPolicy(), ragged=True))
    plain = _shared_run("plain")
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1]) and off[2] == plain[2]
    assert sorted(off[3]) == sorted(plain[3]) and all(np.array_equal(off[3][e], plain[3][e]) for e in plain[3])


def test_front_end_with_a_policy_equals_host_feeding():
    """The same batches (the epoch tables under the same numpy seed) transformed by rs.transform with the front-end's key chain,
    augmented by augment_batch with the policy's rows and fed through step.step give a bit-identical student; feeding each
    batch the previous batch's parameter rows does not."""
    from dcase2019_task4_amd.augment import augment_batch
    n = 7
    pol = _policy()
    rs = _train_set(pol, ragged=False)
    s_res = _front_end_run(rs, np_seed=77, n=n)[0]
    np.random.seed(77)
    rows = np.concatenate([rs.epoch_table() for _ in range(3)])[:n]
    params = np.concatenate([pol.draw(e, rs.n_steps, rs.stream_slices, rs.frames, rs.target_shape[0], rs.n_mels) for e in range(3)])[:n]
    k0 = (rs.seed * PHI + 0x2545F4914F6CDD1D) & 0x7FFFFFFFFFFFFFFF
    keys = [(k0 + (k + 1) * PHI) & (2 ** 64 - 1) for k in range(n)]
    keys = [k - 2 ** 64 if k >= 2 ** 63 else k for k in keys]

    def host(lag):
        st, s, _ = _mt_step(rs)
        for k in range(n):
            x, x_ema, tgt = rs.transform(rows[k], seed=keys[k])
            st.step(*augment_batch(x, x_ema, tgt, params[max(0, k - lag)]))
        torch.cuda.synchronize()
        st.close()
        return s._flat.clone()

    assert torch.equal(s_res, host(0))
    assert not torch.equal(s_res, host(1))

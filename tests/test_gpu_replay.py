"""-m gpu test of sed_kernel_replay (csrc/crnn.hip): every stage of the specialised fp32 step, re-launched alone on the buffers
of a real step, has to put back exactly what the step itself left there.  bench.py's roofline table and the tuning tools time
kernels through this entry, and the step, the backward and the replay bind the same launchers: a pointer that differs between
them shows up here as a buffer that does not come back."""
import ctypes as C
import types

import pytest
import torch

from oracle import synth
from tests import gpu_util as gu
from tests.test_gpu_parity import _check_grads

pytestmark = pytest.mark.gpu

B, T = 4, 128
SEPARATE_HEADS = 1 << 24      # SED_DEBUG_SEPARATE_HEADS (include/dcase_sed.h)
# every name of sed_kernel_replay but gru_wgrad (tests/test_gpu_gru_wgrad.py)
STAGES = ["x_moments", "blk0_fwd", "conv1_fwd", "glu1_fwd", "conv2_fwd", "glu2_fwd", "gru0_fwd", "gru1_fwd", "heads_fwd",
          "gru1_bwd", "gru0_bwd", "glu2_bwd", "conv2_wgrad", "conv2_dgrad", "glu1_bwd", "conv1_wgrad", "conv1_dgrad", "blk0_bwd"]
# the sed_crnn_ctx_view regions a stage writes
CTX_OUT = {"blk0_fwd": ["p0"], "conv1_fwd": ["y1"], "conv2_fwd": ["y2"], "glu1_fwd": ["p1"], "glu2_fwd": ["p2"],
           "gru0_fwd": ["gru0", "gates0"], "gru1_fwd": ["gru1", "gates1"], "heads_fwd": ["logits_s", "den"]}
# the parameters whose gradient a stage writes, as positions in block i's six (conv w, conv b, bn gamma, bn beta, glu w, glu b)
GRAD_OUT = {"conv1_wgrad": (1, [0]), "conv2_wgrad": (2, [0]), "glu1_bwd": (1, [1, 2, 3, 4, 5]), "glu2_bwd": (2, [1, 2, 3, 4, 5]),
            "blk0_bwd": (0, [0, 1, 2, 3, 4, 5])}
# ... out of fp64 sums that the replay accumulates again with atomics: compared under the gradient rule, not bit for bit
ATOMIC_GRADS = {"glu1_bwd", "glu2_bwd", "blk0_bwd"}
ATOMIC_CTX = {"conv1_fwd": "stat1", "conv2_fwd": "stat2"}
# How many bytes of the workspace such a stage may leave different: its fp64 accumulators (+ the 192 BatchNorm-backward
# coefficients derived from them) - csrc/common.h SED_GLUACC_N = 4296, WsLayout::coef; 2 x 64 x 10 sums of block 0.  Everything
# else the stage writes there (dz: 128 KiB and 1 MiB at this shape) comes back bit for bit.  None: not compared.
WS_MAY_DIFFER = {"glu1_bwd": 4296 * 8 + 192 * 4, "glu2_bwd": 4296 * 8 + 192 * 4, "blk0_bwd": 2 * 64 * 10 * 8, "conv2_wgrad": None}


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _view(st, name):
    off, nb = C.c_size_t(), C.c_size_t()
    from dcase2019_task4_amd import _lib
    _lib.check(st.l.sed_crnn_ctx_view(C.byref(st.dims), name.encode(), C.byref(off), C.byref(nb)), "sed_crnn_ctx_view")
    assert 0 < nb.value and off.value + nb.value <= st.ctx_bytes
    return off.value, off.value + nb.value


@pytest.fixture(scope="module")
def snap():
    """One eager mean-teacher step with the heads as kernels of their own (SED_DEBUG_SEPARATE_HEADS: the fused form keeps the
    top layer's d_out in LDS and runs no k_heads_fwd, so there would be nothing for gru1_bwd / heads_fwd to be compared with), and
    what the replays need that the step itself moves on: the parameters before Adam and the step state with this step's seed."""
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.train import MeanTeacherStep
    student, teacher = gu.make_model(0, dropout=0.5)[0], gu.make_model(1, dropout=0.5)[0]
    student.train()
    teacher.train()
    tgt, wm, sm = synth.make_target(3, B, T // 8)
    st = MeanTeacherStep(student, teacher, B, T, 150, wm, sm, seed=99, use_graph=False)
    st.load_batch(synth.make_input(60, B, T).cuda(), synth.make_input(70, B, T).cuda(), tgt.cuda())
    torch.cuda.synchronize()
    params, state = st.student._flat.clone(), st.state.clone()
    old = st.l.sed_debug_set(SEPARATE_HEADS)
    try:
        st.run()
        torch.cuda.synchronize()
    finally:
        st.l.sed_debug_set(old)
    st.check_health()
    assert bool(torch.isfinite(st.grads).all())
    names = [n for n, _ in st.student.named_parameters()]
    offs = _lib.param_layout(st.dims)
    assert len(offs) == len(names) + 1
    return types.SimpleNamespace(st=st, params=params, names=names, offs=offs,
                                 seed=C.c_void_p(state.data_ptr() + _lib.SedStepState.seed_student.offset), state=state,
                                 ctx=st.ctx_s.clone(), ws=st.ws.clone(), grads=st.grads.clone())


def _replay(s, name, dims=None):
    from dcase2019_task4_amd import _lib
    st = s.st
    rc = st.l.sed_kernel_replay(name.encode(), C.byref(dims if dims is not None else st.dims), _lib.ptr(s.params), _lib.ptr(st.x),
                                s.seed, _lib.ptr(st.ctx_s), st.ctx_bytes, _lib.ptr(st.grads), _lib.ptr(st.ws), st.ws_bytes,
                                _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", STAGES)
def test_replayed_stage_restores_what_the_step_left(snap, name):
    """Each stage: the three buffers restored from the snapshot, the stage's addressable outputs overwritten with NaN, one replay,
    everything compared with the snapshot.

    Bit for bit - the kernel's value depends on its inputs alone: x_moments (per-workgroup partials, no reduction across
    workgroups), blk0_fwd, glu{i}_fwd, gru{l}_fwd, heads_fwd, gru{l}_bwd, conv{i}_dgrad, conv{i}_wgrad (partial slabs + a
    fixed-order reduce, "deterministic, no atomics": conv.hip), the y of conv{i}_fwd and the dz of glu{i}_bwd.
    Under the gradient rule (_check_grads: 1e-3 of the typical magnitude) - the value is re-formed through fp64 atomicAdd, whose
    order is not fixed: the BatchNorm sums stat{i} that k_conv*'s epilogue adds per wave (conv.hip) and a conv{i}_fwd replay
    clears and accumulates again; the five parameter gradients k_bn_bwd_prep derives from the accumulators of k_glu_pool_bwd8
    (bnglu.hip: dW_glu, db_glu, sum dz, sum dz y); the six that k_blk0_bwd_finalize derives from the sums of k_blk0_bwd (blk0.hip).
    Those stages' accumulators (and coefficients) are also all that may differ in the workspace.
    conv2_wgrad's workspace is not compared: the partial slabs are shared and hold block 1's after a step."""
    st = snap.st
    st.ctx_s.copy_(snap.ctx)
    st.ws.copy_(snap.ws)
    st.grads.copy_(snap.grads)
    for v in CTX_OUT.get(name, []) + ([ATOMIC_CTX[name]] if name in ATOMIC_CTX else []):
        lo, hi = _view(st, v)
        st.ctx_s[lo:hi] = 0xFF               # (a NaN in fp32 and fp64)
    blk, which = GRAD_OUT.get(name, (0, []))
    out = [6 * blk + k for k in which]
    for i in out:
        st.grads[snap.offs[i]:snap.offs[i + 1]] = float("nan")
    assert _replay(snap, name) == 0, st.l.sed_last_error()

    # ---- ctx -----------------------------------------------------------------------------------
    got = st.ctx_s.clone()
    if name in ATOMIC_CTX:
        lo, hi = _view(st, ATOMIC_CTX[name])
        stat, want = got[lo:hi].clone().view(torch.float64).cpu(), snap.ctx[lo:hi].clone().view(torch.float64).cpu()
        _check_grads({ATOMIC_CTX[name]: stat}, {ATOMIC_CTX[name]: want})
        got[lo:hi] = snap.ctx[lo:hi]
    assert torch.equal(got, snap.ctx), "ctx"
    # ---- grads ---------------------------------------------------------------------------------
    got = st.grads.clone()
    if name in ATOMIC_GRADS:
        _check_grads({snap.names[i]: got[snap.offs[i]:snap.offs[i + 1]].cpu() for i in out},
                     {snap.names[i]: snap.grads[snap.offs[i]:snap.offs[i + 1]].cpu() for i in out})
        for i in out:
            got[snap.offs[i]:snap.offs[i + 1]] = snap.grads[snap.offs[i]:snap.offs[i + 1]]
    assert torch.equal(_bits(got), _bits(snap.grads)), "grads"
    # ---- ws ------------------------------------------------------------------------------------
    may = WS_MAY_DIFFER.get(name, 0)
    if may is not None:
        n_diff = int((st.ws != snap.ws).sum())
        print(f"[replay] {name}: {n_diff} workspace bytes differ (allowed {may})")
        assert n_diff <= may, "ws"


def test_replay_errors(snap):
    from dcase2019_task4_amd import _lib
    st = snap.st
    assert _replay(snap, "no_such_kernel") != 0
    assert b"unknown kernel 'no_such_kernel'" in st.l.sed_last_error()
    for kw in (dict(C_=128), dict(H=256), dict(dtype=_lib.DTYPE_BF16)):
        assert _replay(snap, "blk0_fwd", _lib.make_dims(B, T, **kw)) != 0
        assert b"only the C = 64 / H = 64 / fp32 kernel set is replayable" in st.l.sed_last_error()

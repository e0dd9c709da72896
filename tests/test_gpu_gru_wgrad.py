"""-m gpu tests of k_gru_wgrad (csrc/gruw.hip): every weight / bias gradient of the 64-cell fp32 BiGRU from one split-K
launch whose MFMA operands come straight from global memory, plus its fixed-order reduce."""
import ctypes as C

import pytest
import torch

from oracle import synth
from tests import gpu_util as gu
from tests.test_gpu_parity import _check_grads, _fwd_bwd_both

pytestmark = pytest.mark.gpu


# K = B * (T // 8) rows are cut into 16 slices of whole 64-row tiles (4 workgroups x 4 waves per half of a 64 x 64 tile)
@pytest.mark.parametrize("B,T,n_layers", [(1, 16, 2),      # K = 2: less than any slice, almost every slice empty
                                          (3, 40, 2),      # K = 15: odd
                                          (5, 136, 2),     # K = 85: not a multiple of the slice
                                          (2, 1040, 2),    # K = 260
                                          (4, 628, 2),     # K = 312
                                          (5, 216, 1)])    # K = 135: one layer only, odd
def test_gru_weight_gradients_vs_oracle(B, T, n_layers):
    """Every gradient against the oracle under the project's rule (1e-3 of the typical magnitude, measured <= 2e-4), dropout 0.5."""
    hip, orc = _fwd_bwd_both(B, T, 0.5, seed=123456789, n_layers=n_layers)
    gru = [n for n in orc[3] if n.startswith("rnn.rnn.")]
    assert len(gru) == 8 * n_layers
    for n in gru:
        g = orc[3][n]
        typ = float(g.double().norm()) / g.numel() ** 0.5
        print(f"[gru_wgrad] B {B} T {T} {n:32s} err/typ {float((hip[3][n] - g).abs().max()) / (typ + 1e-30):.3e}")
    _check_grads(hip[3], orc[3])


def _step(B, T, seed=99):
    from dcase2019_task4_amd.train import MeanTeacherStep
    student, teacher = gu.make_model(0, dropout=0.5)[0], gu.make_model(1, dropout=0.5)[0]
    student.train()
    teacher.train()
    tgt, wm, sm = synth.make_target(3, B, T // 8)
    st = MeanTeacherStep(student, teacher, B, T, 150, wm, sm, seed=seed, use_graph=False)
    st.load_batch(synth.make_input(60, B, T).cuda(), synth.make_input(70, B, T).cuda(), tgt.cuda())
    st.run()
    torch.cuda.synchronize()
    st.check_health()
    return st


def _gru_slices(st):
    from dcase2019_task4_amd import _lib
    offs = _lib.param_layout(st.dims)
    names = [n for n, _ in st.student.named_parameters()]
    assert len(offs) == len(names) + 1
    sl = [(offs[i], offs[i + 1]) for i, n in enumerate(names) if n.startswith("rnn.rnn.")]
    assert len(sl) == 16
    return sl


def test_replay_restores_the_gru_gradients_bit_for_bit_and_touches_nothing_else():
    from dcase2019_task4_amd import _lib
    st = _step(4, 128)
    want = st.grads.clone()
    for lo, hi in _gru_slices(st):
        st.grads[lo:hi] = float("nan")
    assert not torch.equal(st.grads, want)

    def replay():
        _lib.check(st.l.sed_kernel_replay(b"gru_wgrad", C.byref(st.dims), _lib.ptr(st.student._flat), _lib.ptr(st.x), st._seed_s,
                                          _lib.ptr(st.ctx_s), st.ctx_bytes, _lib.ptr(st.grads), _lib.ptr(st.ws), st.ws_bytes,
                                          _lib.stream_ptr()), "gru_wgrad")
        torch.cuda.synchronize()

    replay()
    # (bit patterns: the step's own gradients hold no NaN - check_health - so torch.equal is a bit-for-bit comparison)
    assert torch.equal(st.grads, want)
    for _ in range(5):
        replay()
        assert torch.equal(st.grads, want)


def test_poisoned_workspace_leaves_the_gru_gradients_finite(monkeypatch):
    """Every ctx / workspace byte starts as 0xFF (NaN): rows past the end of a K slice are selected to zero, never multiplied."""
    monkeypatch.setenv("SED_POISON", "1")
    st = _step(3, 40)
    for lo, hi in _gru_slices(st):
        assert bool(torch.isfinite(st.grads[lo:hi]).all()), (lo, hi)

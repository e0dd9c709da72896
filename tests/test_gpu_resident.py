"""-m gpu tests of training / validation from HBM-resident features: sed_gather_logmel_transform against the numpy oracle
and against sed_logmel_transform, the one-batch-ahead resident front-end against the serial order and against host
feeding, train() and get_predictions with resident sets."""
import numpy as np
import pandas as pd
import pytest
import torch

from oracle import features_np, philox
from oracle import postprocess_np as pp
from tests import gpu_util as gu

pytestmark = pytest.mark.gpu
PHI = 0x9E3779B97F4A7C15


def _clips(lengths, seed=0, n_mels=64):
    rs = np.random.RandomState(seed)
    return [(np.abs(rs.standard_normal((n, n_mels))) * 3.0).astype(np.float32) for n in lengths]


def _scaler(feats, T):
    from dcase2019_task4_amd.features import Scaler
    sc = Scaler()
    sc.calculate_scaler([features_np.transform_chain(f, T) for f in feats[:4]])
    return sc


def _signed(k):
    k &= 2 ** 64 - 1
    return k - 2 ** 64 if k >= 2 ** 63 else k


def _keys(seed, n):
    """The front-end's key chain: extraction k draws with key_0 + (k + 1) strides (features.OneBatchAheadFrontEnd)."""
    k0 = (seed * PHI + 0x2545F4914F6CDD1D) & 0x7FFFFFFFFFFFFFFF
    return [_signed(k0 + (k + 1) * PHI) for k in range(n)]


def test_gather_transform_vs_oracle_ragged_clips():
    """Clips shorter than, equal to and longer than max_frames, one with 1e-7 rows (the top-db floor), gathered with repeats
    and out of order: features against transform_chain with the noise of counter b * L_max * 64 + e, targets exact."""
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    T = 628
    lengths = [600, 628, 650, 301, 628]
    feats = _clips(lengths, 11)
    feats[0][5, :] *= 1e-7
    feats[3][:, :] *= 1e-7
    feats[3][7, :] = 2.0
    tgts = [np.random.RandomState(50 + i).uniform(-1, 1, size=(T // 8, 10)).astype(np.float32) for i in range(5)]
    sc = _scaler(feats, T)
    idx = [2, 0, 2, 4, 1, 3]
    seed = 987654321
    noise = philox.teacher_noise(seed, len(idx), max(lengths), 64)
    res = {}
    for md in ("f64", "f32"):
        rs = ResidentFeatureSet.from_arrays(feats, tgts, frames=T, scaler=sc, math_dtype=md)
        clean, noisy, tgt = rs.transform(idx, seed=seed)
        assert clean.shape == noisy.shape == (len(idx), 1, T, 64) and tgt.shape == (len(idx), T // 8, 10)
        np.testing.assert_array_equal(tgt.cpu().numpy(), np.stack([tgts[i] for i in idx]))
        res[md] = clean, noisy
    c, n = res["f64"]
    for b, i in enumerate(idx):
        wc, wn = features_np.transform_chain(feats[i], T, sc.mean_, sc.std_, noise[b, :lengths[i]].astype(np.float64))
        ec, en = np.abs(c[b].cpu().numpy() - wc).max(), np.abs(n[b].cpu().numpy() - wn).max()
        print(f"[gather] position {b} clip {i} ({lengths[i]} frames): clean err {ec:.2e} noisy err {en:.2e}")
        np.testing.assert_allclose(c[b].cpu().numpy(), wc, atol=2e-5)
        np.testing.assert_allclose(n[b].cpu().numpy(), wn, atol=2e-5)
    # the stated fp32 mode: 2e-4 of the per-band std against the float64 mode (tests/test_gpu_features.py)
    ec, en = (res["f32"][0] - c).abs().max().item(), (res["f32"][1] - n).abs().max().item()
    print(f"[gather] f32 mode: clean {ec:.2e} noisy {en:.2e}")
    assert ec < 2e-4 and en < 2e-4


@pytest.mark.parametrize("math_dtype", ["f64", "f32"])
def test_gather_equal_length_pool_is_bit_identical_to_logmel_transform(math_dtype):
    from dcase2019_task4_amd.features import LogMelTransform
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    T, L = 628, 640
    feats = _clips([L] * 6, 3)
    sc = _scaler(feats, T)
    idx = [4, 1, 1, 5, 0]
    stacked = torch.tensor(np.stack([feats[i] for i in idx])).cuda()
    seed = _signed(0xDEADBEEF12345678 + PHI)
    rs = ResidentFeatureSet.from_arrays(feats, None, frames=T, scaler=sc, math_dtype=math_dtype)
    clean, noisy, tgt = rs.transform(idx, seed=seed)
    assert tgt is None
    wc, wn = LogMelTransform(T, sc, augment_type="noise", math_dtype=math_dtype)(stacked, seed=seed)
    assert torch.equal(clean, wc) and torch.equal(noisy, wn)
    ev = ResidentFeatureSet.from_arrays(feats, None, frames=T, scaler=sc, augment_type=None, math_dtype=math_dtype)
    (vc, _) = ev.transform(idx)
    assert torch.equal(vc, LogMelTransform(T, sc, math_dtype=math_dtype)(stacked)) and torch.equal(vc, clean)


def _train_set(lengths_seed=0, ragged=True, T=628, lengths=(560, 700)):
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    sizes, bsz = (8, 12, 8), (2, 4, 2)                      # 3 steps per epoch (min(8 // 2, 12 // 4, 8 // 2))
    rs_ = np.random.RandomState(lengths_seed)
    lengths = [int(rs_.randint(*lengths)) if ragged else T for _ in range(sum(sizes))]
    feats = _clips(lengths, 20 + lengths_seed)
    tgts = []
    for i in range(sum(sizes)):
        r = np.random.RandomState(300 + i)
        if i < sizes[0]:
            tgts.append(np.repeat((r.uniform(size=(1, 10)) < 0.3).astype(np.float32), T // 8, axis=0))
        elif i < sizes[0] + sizes[1]:
            tgts.append(-np.ones((T // 8, 10), np.float32))
        else:
            tgts.append((r.uniform(size=(T // 8, 10)) < 0.2).astype(np.float32))
    sc = _scaler(feats, T)
    return ResidentFeatureSet.from_arrays(feats, tgts, sizes, bsz, frames=T, scaler=sc, seed=5), feats, tgts, sc


def _mt_step(rs, seed=99, mfma_dtype="f32"):
    from dcase2019_task4_amd.train import MeanTeacherStep
    student, _ = gu.make_model(0, dropout=0.5, mfma_dtype=mfma_dtype)
    teacher, _ = gu.make_model(1, dropout=0.5, mfma_dtype=mfma_dtype)
    student.train(); teacher.train()
    st = MeanTeacherStep(student, teacher, rs.batch, rs.frames, 100, rs.weak_mask, rs.strong_mask, seed=seed, use_graph=True)
    return st, student, teacher


@pytest.mark.parametrize("fe_moments", [None, "1"], ids=["default", "moments"])
def test_resident_front_end_one_batch_ahead_equals_serial_across_epochs(fe_moments, monkeypatch):
    """7 steps over 3-step epochs (two epoch boundaries, the second table drawn while the first epoch runs): the gather of
    batch k + 1 inside step k's hipGraph must leave models and meters bit-identical to the serial protocol.  SED_FE_MOMENTS=1:
    the front-end also writes block 0's patch moments of batch k + 1 (off by default in fp32) - through the eager steps, the
    capture, both slots' graphs and the serial protocol's own graph."""
    from dcase2019_task4_amd.resident import ResidentFrontEnd
    if fe_moments is None:
        monkeypatch.delenv("SED_FE_MOMENTS", raising=False)
    else:
        monkeypatch.setenv("SED_FE_MOMENTS", fe_moments)
    rs = _train_set()[0]
    out = []
    for overlap in (False, True):
        np.random.seed(2024)
        st, s, t = _mt_step(rs)
        fe = ResidentFrontEnd(st, rs, overlap=overlap)
        assert fe.overlap == overlap and fe.moments == (fe_moments == "1")
        meters = []
        for _ in range(7):
            fe.run()
            meters.append(st.meters())
        assert st.steps_done == 7 and fe._epoch == 2 and fe._pos == 2
        out.append((s._flat.clone(), t._flat.clone(), meters))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and all(np.isfinite(m["loss"]) for m in out[0][2])


def test_resident_front_end_f16_with_moments_tracks_serial_without(monkeypatch):
    """The same 7 steps in the fp16-forward mode, where the front-end owns the moments by default: the overlap protocol with
    them against the serial protocol with SED_FE_MOMENTS=0 (every forward computes its own), same dropout keys, on the
    student's strong and weak posteriors of every step.  Each leg is within F16_POST_TOL of the exact value, so they are
    within twice that of each other."""
    from dcase2019_task4_amd.resident import ResidentFrontEnd
    from tests.test_gpu_generic import F16_POST_TOL
    rs = _train_set()[0]
    out = []
    for overlap, env in ((False, "0"), (True, None)):
        if env is None:
            monkeypatch.delenv("SED_FE_MOMENTS", raising=False)
        else:
            monkeypatch.setenv("SED_FE_MOMENTS", env)
        np.random.seed(2024)
        st, s, t = _mt_step(rs, mfma_dtype="f16")
        fe = ResidentFrontEnd(st, rs, overlap=overlap)
        assert fe.overlap == overlap and fe.moments == (env is None)
        post = []
        for _ in range(7):
            fe.run()
            post.append((st.strong.clone(), st.weak.clone()))
        torch.cuda.synchronize()
        out.append(post)
    for k, ((s0, w0), (s1, w1)) in enumerate(zip(*out)):
        es, ew = float((s0 - s1).abs().max()), float((w0 - w1).abs().max())
        print(f"[resident f16] step {k}: overlap + moments against serial without: strong {es:.2e} weak {ew:.2e}")
        assert torch.isfinite(s1).all() and es < 2 * F16_POST_TOL and ew < 2 * F16_POST_TOL, (k, es, ew)


def test_resident_feeding_equals_host_feeding():
    """The same batches (the epoch tables under the same numpy seed), transformed by LogMelTransform with the front-end's key
    sequence and fed through step.step, give bit-identical models; feeding each batch with the previous batch's target
    does not."""
    from dcase2019_task4_amd.features import LogMelTransform
    from dcase2019_task4_amd.resident import ResidentFrontEnd
    rs, feats, tgts, sc = _train_set(1, ragged=False)
    n = 7
    np.random.seed(77)
    st, s_res, _ = _mt_step(rs)
    fe = ResidentFrontEnd(st, rs)
    for _ in range(n):
        fe.run()
    torch.cuda.synchronize()
    np.random.seed(77)
    rows = np.concatenate([rs.epoch_table() for _ in range(3)])[:n]
    keys = _keys(rs.seed, n)
    tr = LogMelTransform(rs.frames, sc, augment_type="noise")
    feats_t = torch.tensor(np.stack(feats)).cuda()
    tgts_t = torch.tensor(np.stack(tgts)).cuda()

    def host(lag):
        st, s, _ = _mt_step(rs)
        for k in range(n):
            r = torch.tensor(rows[k]).long().cuda()
            x, x_ema = tr(feats_t[r], seed=keys[k])
            st.step(x, x_ema, tgts_t[torch.tensor(rows[max(0, k - lag)]).long().cuda()])
        torch.cuda.synchronize()
        return s._flat.clone()

    assert torch.equal(s_res._flat, host(0))
    assert not torch.equal(s_res._flat, host(1))


def test_train_with_a_resident_set():
    from dcase2019_task4_amd.resident import ResidentFeatureSet, ResidentFrontEnd
    from dcase2019_task4_amd.train import MeanTeacherStep, train
    rs = _train_set(2)[0]
    student, _ = gu.make_model(0, dropout=0.5)
    teacher, _ = gu.make_model(1, dropout=0.5)
    opt = torch.optim.Adam(student.parameters(), lr=1e-3, betas=(0.9, 0.999))
    lines = []
    np.random.seed(5)
    m0 = train(rs, student, opt, 0, ema_model=teacher, weak_mask=rs.weak_mask, strong_mask=rs.strong_mask, log=lines.append)
    st = student._mt_step
    assert st.steps_done == 3 and st.read_state().global_step == 3
    m1 = train(rs, student, opt, 1, ema_model=teacher, weak_mask=rs.weak_mask, strong_mask=rs.strong_mask, log=lines.append)
    assert st.steps_done == 6 and st.read_state().global_step == 6 and st.global_step_host == 6
    assert lines[0].startswith("Epoch: 0\tTime ") and lines[1].startswith("Epoch: 1\tTime ") and "cons_weight" in lines[1]
    # the same sequence through the front-end by hand (what train() wraps)
    s2, _ = gu.make_model(0, dropout=0.5)
    t2, _ = gu.make_model(1, dropout=0.5)
    np.random.seed(5)
    st2 = MeanTeacherStep(s2, t2, rs.batch, rs.frames, 3 * 100 // 2, rs.weak_mask, rs.strong_mask, lr=1e-3)
    fe = ResidentFrontEnd(st2, rs)
    want = []
    for _ in range(2):
        for _ in range(3):
            fe.run()
        want.append(st2.meters())
    assert [m0, m1] == want and all(np.isfinite(m["loss"]) for m in want)
    assert torch.equal(student._flat, s2._flat) and torch.equal(teacher._flat, t2._flat)
    # main_simple_CRNN: no teacher, no noise
    feats, tgts = _clips([628] * 16, 9), [np.zeros((78, 10), np.float32)] * 16
    sup = ResidentFeatureSet.from_arrays(feats, tgts, (8, 8), (2, 2), frames=628, augment_type=None)
    model, _ = gu.make_model(3, dropout=0.5)
    m = train(sup, model, torch.optim.Adam(model.parameters(), lr=1e-3), 0, weak_mask=sup.weak_mask, log=lambda s: None)
    assert model._mt_step.steps_done == 4 and np.isfinite(m["loss"])


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


def test_get_predictions_resident_equals_per_clip():
    from dcase2019_task4_amd.features import LogMelTransform
    from dcase2019_task4_amd.inference import get_predictions
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    T = 628
    feats = _clips([628, 500, 700, 628, 640, 300, 628], 4)
    for k, f in enumerate(feats):
        f *= 1.0 + 2.0 * (k % 3)
    sc = _scaler(feats, T)
    tr = LogMelTransform(T, sc)
    per_clip = _DS([tr(torch.tensor(f)[None])[0].cpu() for f in feats])
    res = ResidentFeatureSet.for_eval(_EvalDS(feats), T, sc)
    assert len(res) == 7 and res.filenames.tolist() == per_clip.filenames.tolist()
    model, _ = gu.make_model(2)
    model.eval()
    dec = type("Enc", (), {"labels": [f"c{i}" for i in range(10)], "decode_strong": lambda self, m: pp.decode_strong(m, self.labels)})()
    for bs in (3, 64):
        want = get_predictions(model, per_clip, dec.decode_strong, 8, batch_size=bs)
        got = get_predictions(model, res, dec.decode_strong, 8, batch_size=bs)
        assert len(want) > 0
        pd.testing.assert_frame_equal(got, want)


def test_gather_argument_checks_on_real_buffers():
    """sed_gather_logmel_transform refuses sizes it cannot address.  Every buffer is real and large enough for the launch these
    arguments describe (all indices 0, one frame of one band, no noise), so even a check that stopped working could not read or
    write outside them."""
    from dcase2019_task4_amd import _lib
    l = _lib.lib()
    B = 4096
    dev = dict(device="cuda")
    pool = torch.ones(1, dtype=torch.float32, **dev)
    off = torch.zeros(1, dtype=torch.int64, **dev)
    frames = torch.ones(1, dtype=torch.int32, **dev)
    idx = torch.zeros(B, dtype=torch.int32, **dev)
    out = torch.empty(B, dtype=torch.float32, **dev)
    tgt = torch.zeros(1, dtype=torch.float32, **dev)
    ws = torch.empty(l.sed_logmel_transform_ws_bytes(B), dtype=torch.uint8, **dev)
    P = _lib.ptr

    def call(max_clip_frames, b, tgt_pool=None, tgt_elems=0, out_target=None, ws_bytes=None):
        return l.sed_gather_logmel_transform(P(pool), P(off), P(frames), 1, max_clip_frames, P(idx), b, 1, 1, None, None, None,
                                             P(out), None, P(tgt_pool), tgt_elems, P(out_target), P(ws),
                                             ws.numel() if ws_bytes is None else ws_bytes, 0, _lib.stream_ptr())

    assert call(1 << 20, B) != 0 and b"noise stream" in l.sed_last_error()        # B x L_max x n_mels = 2^32
    assert call(1, 0) != 0 and b"bad sizes" in l.sed_last_error()
    assert call(1, 2, tgt, 0, out) != 0 and b"tgt_elems" in l.sed_last_error()
    assert call(1, 2, tgt, 1, None) != 0 and b"go together" in l.sed_last_error()
    assert call(1, B, ws_bytes=16) != 0 and b"workspace" in l.sed_last_error()
    torch.cuda.synchronize()
    assert call(1, 2) == 0                                                         # and the same buffers are a valid launch
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[:2].cpu().numpy(), [0.0, 0.0])               # 10 log10(1) = 0 dB

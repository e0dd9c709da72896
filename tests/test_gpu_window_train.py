"""-m gpu tests of training on windows of long pool items: sed_gather_window_logmel_transform bit for bit against the merged
gather on the same windows cut on the host (tests/window_np.py), its clamps and argument checks, the resident front-end over
a WindowedFeatureSet against the serial order and against host feeding, augmentation, train(), and the plain set's front-end
left as it was."""
import types

import numpy as np
import pytest
import torch

from oracle import features_np
from tests import augment_np
from tests import gpu_util as gu
from tests import window_np as wn

pytestmark = pytest.mark.gpu
PHI = 0x9E3779B97F4A7C15
FRAMES, POOL = 32, 4
LENGTHS = [1, 31, 32, 33, 100, 259]
# the same item at different starts, start3 = 0, the last start the label rule allows (56) and the last legal one (64: three
# real frames), short items, one-frame windows
WINDOWS = [(5, 0), (5, 56), (4, 17), (5, 30), (0, 0), (4, 3), (1, 0), (1, 7), (5, 64), (2, 0), (3, 0), (3, 8), (4, 0)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _items(n_mels, nclass, seed=0):
    rs = np.random.RandomState(seed)
    feats = [(np.abs(rs.standard_normal((n, n_mels))) * 3.0).astype(np.float32) for n in LENGTHS]
    feats[4][20:70] *= 1e-7                                       # the top-dB floor bites in the windows that hold a loud frame too
    labels = [rs.uniform(-1, 1, size=(max(1, n // POOL), nclass)).astype(np.float32) for n in LENGTHS]
    labels[1][:] = -1.0                                           # the unlabelled stream's rows
    sc = types.SimpleNamespace(mean_=rs.uniform(-30, -10, n_mels), std_=rs.uniform(5, 15, n_mels))
    return feats, labels, sc


def _poisoned(*shape):
    return torch.full(shape, -1, device="cuda", dtype=torch.int32).view(torch.float32)          # NaN bytes


def _gather(rset, table, seed, T3, nclass):
    """rset.gather into buffers that start as NaN bytes -> (clean, noisy or None, target)."""
    table = torch.tensor(np.asarray(table, dtype=np.int32)).cuda()
    B = table.shape[0]
    clean = _poisoned(B, 1, rset.frames, rset.n_mels)
    noisy = _poisoned(B, 1, rset.frames, rset.n_mels) if rset.noise else None
    key = torch.tensor([seed], dtype=torch.int64, device="cuda") if rset.noise else None
    tgt = _poisoned(B, T3, nclass)
    rset.gather(table, clean, noisy, key, tgt)
    torch.cuda.synchronize()
    return clean, noisy, tgt


@pytest.mark.parametrize("noise", [True, False], ids=["noise", "clean"])
@pytest.mark.parametrize("math_dtype", ["f64", "f32"])
@pytest.mark.parametrize("nclass", [3, 10])
@pytest.mark.parametrize("n_mels", [8, 5])
def test_window_gather_is_bit_identical_to_the_merged_gather_on_host_cut_windows(n_mels, nclass, math_dtype, noise):
    from dcase2019_task4_amd.longrec import WindowedFeatureSet
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    feats, labels, sc = _items(n_mels, nclass)
    kw = dict(scaler=sc, augment_type="noise" if noise else None, math_dtype=math_dtype)
    ws = WindowedFeatureSet.from_arrays(feats, labels, [3, 3], [1, 1], FRAMES, [False, True], pooling_time_ratio=POOL, **kw)
    cuts = [wn.cut_window(feats[i], labels[i], s, FRAMES, POOL) for i, s in WINDOWS]
    assert max(c[0].shape[0] for c in cuts) == FRAMES == ws.max_win_frames        # a full window: both noise strides are 32 * n_mels
    assert min(c[0].shape[0] for c in cuts) == 1
    plain = ResidentFeatureSet.from_arrays([c[0] for c in cuts], [c[1] for c in cuts], frames=FRAMES, **kw)
    seed = 0x1234567 + 977 * n_mels
    T3 = FRAMES // POOL
    got = _gather(ws, WINDOWS, seed, T3, nclass)
    want = _gather(plain, np.arange(len(WINDOWS)), seed, T3, nclass)
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.isfinite(got[0]).all()
    assert torch.equal(_bits(got[2]), _bits(want[2]))
    np.testing.assert_array_equal(got[2].cpu().numpy(), np.stack([c[1] for c in cuts]))
    if noise:
        assert torch.equal(_bits(got[1]), _bits(want[1])) and not torch.equal(got[1], got[0])
    # the convenience form checks its table and gives the same bytes
    out = ws.transform(WINDOWS, seed=seed if noise else None)
    assert torch.equal(out[0], got[0]) and torch.equal(out[-1], got[2])


def test_the_clamp_is_the_windows_own():
    """A frame 60 dB above everything else, outside the window: no byte of the window's output changes.  Inside it: it does."""
    from dcase2019_task4_amd.longrec import WindowedFeatureSet
    feats, labels, sc = _items(8, 3, 1)
    loud = [f.copy() for f in feats]
    loud[5][7] *= 1e3                                             # item 5, frame 7
    win = [(5, 2), (5, 30), (5, 64), (5, 0), (5, 1)]              # frames 8.., 120.., 256..: outside; 0.., 4..: inside
    out = []
    for f in (feats, loud):
        ws = WindowedFeatureSet.from_arrays(f, labels, [6], [1], FRAMES, [True], pooling_time_ratio=POOL, scaler=sc)
        out.append(_gather(ws, win, 99, FRAMES // POOL, 3))
    for k in range(3):
        assert torch.equal(_bits(out[0][k][:3]), _bits(out[1][k][:3]))
    assert not torch.equal(out[0][0][3], out[1][0][3]) and not torch.equal(out[0][0][4], out[1][0][4])


def test_window_gather_argument_checks_and_clamped_tables():
    """sed_gather_window_logmel_transform refuses what it cannot address; every buffer is real and large enough for the launch
    the arguments describe.  Table content outside the pool is clamped inside the kernel (item to [0, n_pool), start3 to the
    item's last frame - reviewed in LmWindow: every address is formed from the clamped values only), so such rows give the
    clamped windows' outputs."""
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.longrec import WindowedFeatureSet
    l = _lib.lib()
    B = 4096
    dev = dict(device="cuda")
    pool = torch.ones(1, dtype=torch.float32, **dev)
    off = torch.zeros(1, dtype=torch.int64, **dev)
    frames = torch.ones(1, dtype=torch.int32, **dev)
    win = torch.zeros(B, 2, dtype=torch.int32, **dev)
    out = torch.empty(B, dtype=torch.float32, **dev)
    lab = torch.full((1,), 0.5, dtype=torch.float32, **dev)
    rows = torch.ones(1, dtype=torch.int32, **dev)
    out_t = torch.empty(B, dtype=torch.float32, **dev)
    ws = torch.empty(l.sed_logmel_transform_ws_bytes(B), dtype=torch.uint8, **dev)
    P = _lib.ptr

    def call(max_win_frames, b, pool_ratio=1, labels=(None, None, None, None), ws_bytes=None):
        lp, lo, lr, ot = labels
        return l.sed_gather_window_logmel_transform(P(pool), P(off), P(frames), 1, max_win_frames, P(win), b, 1, 1, pool_ratio,
                                                    None, None, None, P(out), None, P(lp), P(lo), P(lr), 1, 1, P(ot), P(ws),
                                                    ws.numel() if ws_bytes is None else ws_bytes, 0, _lib.stream_ptr())

    assert call(1 << 20, B) != 0 and b"noise stream" in l.sed_last_error()        # B x max_win_frames x n_mels = 2^32
    assert call(1, 0) != 0 and b"bad sizes" in l.sed_last_error()
    assert call(1, 2, pool_ratio=0) != 0 and b"pool_ratio" in l.sed_last_error()
    for half in ((lab, off, rows, None), (lab, None, rows, out_t), (None, off, rows, out_t), (lab, off, None, out_t)):
        assert call(1, 2, labels=half) != 0 and b"go together" in l.sed_last_error()
    assert call(1, B, ws_bytes=16) != 0 and b"workspace" in l.sed_last_error()
    torch.cuda.synchronize()
    assert call(1, 2, labels=(lab, off, rows, out_t)) == 0                         # and the same buffers are a valid launch
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[:2].cpu().numpy(), [0.0, 0.0])               # 10 log10(1) = 0 dB
    np.testing.assert_array_equal(out_t[:2].cpu().numpy(), [0.5, 0.5])
    # clamped rows
    feats, labels, sc = _items(8, 3, 2)
    wset = WindowedFeatureSet.from_arrays(feats, labels, [6], [1], FRAMES, [True], pooling_time_ratio=POOL, scaler=sc)
    big, small = 2 ** 31 - 1, -2 ** 31
    hostile = [(-1, 0), (6, 0), (4, big), (5, -5), (big, big), (small, small), (1, 8)]
    clamped = [(0, 0), (5, 0), (4, 24), (5, 0), (5, 64), (0, 0), (1, 7)]
    got = _gather(wset, hostile, 5, FRAMES // POOL, 3)
    want = _gather(wset, clamped, 5, FRAMES // POOL, 3)
    for g, w in zip(got, want):
        assert torch.isfinite(g).all() and torch.equal(_bits(g), _bits(w))
    with pytest.raises(_lib.SedError):
        wset.transform(hostile[:1], seed=5)                                        # the host refuses such a table
    with pytest.raises(_lib.SedError):
        wset.gather(torch.zeros(4, dtype=torch.int32, device="cuda"), got[0])      # clip indices are not windows
    with pytest.raises(_lib.SedError):
        wset.eval_batch(0, 2)


# ---- the front-end over a windowed set ---------------------------------------------------------------------------------------
T, P8 = 64, 8                        # the smallest clip the fp32 step's tiles are exercised at elsewhere (B = 2 x T = 64)
SIZES, BSZ = (8, 12, 3), (2, 4, 2)   # [weak clips | unlabelled clips | strongly labelled recordings]: 3 steps per epoch
_POOL = {}


def _train_items(full):
    """Two streams of clips (ragged around T, or all at least T frames when ``full``) and three recordings of 150 - 400 frames,
    with timelines; host arrays and the scaler built once."""
    if full not in _POOL:
        from dcase2019_task4_amd.features import Scaler
        rs_ = np.random.RandomState(3 + full)
        lengths = [int(rs_.randint(T, T + 20)) if full else int(rs_.randint(50, 80)) for _ in range(SIZES[0] + SIZES[1])]
        lengths += [152, 260, 400]
        feats = [(np.abs(rs_.standard_normal((n, 64))) * 3.0).astype(np.float32) for n in lengths]
        labels = []
        for i, n in enumerate(lengths):
            r = np.random.RandomState(300 + i)
            if i < SIZES[0]:
                labels.append(np.repeat((r.uniform(size=(1, 10)) < 0.3).astype(np.float32), T // P8, axis=0))
            elif i < SIZES[0] + SIZES[1]:
                labels.append(-np.ones((T // P8, 10), np.float32))
            else:
                labels.append((r.uniform(size=(n // P8, 10)) < 0.2).astype(np.float32))
        sc = Scaler()
        sc.calculate_scaler([features_np.transform_chain(f[:T], T) for f in feats[:4]])
        _POOL[full] = feats, labels, sc
    return _POOL[full]


def _train_set(full=False, augment=None, sampling="random"):
    from dcase2019_task4_amd.longrec import WindowedFeatureSet
    feats, labels, sc = _train_items(full)
    ws = WindowedFeatureSet.from_arrays(feats, labels, SIZES, BSZ, T, [False, False, True], pooling_time_ratio=P8,
                                        sampling=sampling, scaler=sc, seed=5, augment=augment)
    assert ws.n_steps == 3 and ws.batch == 8 and ws.window_stream_sizes == [8, 12, 4 + 7 + 12]
    return ws


def _mt_step(rs, seed=99):
    from dcase2019_task4_amd.train import MeanTeacherStep
    student, _ = gu.make_model(0, dropout=0.5)
    teacher, _ = gu.make_model(1, dropout=0.5)
    student.train(); teacher.train()
    st = MeanTeacherStep(student, teacher, rs.batch, rs.frames, 100, rs.weak_mask, rs.strong_mask, seed=seed, use_graph=True)
    return st, student, teacher


def _signed(k):
    k &= 2 ** 64 - 1
    return k - 2 ** 64 if k >= 2 ** 63 else k


def _keys(seed, n):
    """The front-end's key chain: extraction k draws with key_0 + (k + 1) strides (features.OneBatchAheadFrontEnd)."""
    k0 = (seed * PHI + 0x2545F4914F6CDD1D) & 0x7FFFFFFFFFFFFFFF
    return [_signed(k0 + (k + 1) * PHI) for k in range(n)]


def test_windowed_front_end_one_batch_ahead_equals_serial_across_epochs():
    """7 steps over 3-step epochs, random crops: the window gather of batch k + 1 inside step k's hipGraph leaves models and
    meters bit-identical to the serial protocol; the tables are those of epochs 0, 1, 2 under the same global seed."""
    from dcase2019_task4_amd.resident import ResidentFrontEnd
    ws = _train_set()
    out = []
    for overlap in (False, True):
        np.random.seed(2024)
        st, s, t = _mt_step(ws)
        fe = ResidentFrontEnd(st, ws, overlap=overlap)
        assert fe.overlap == overlap and fe.idx.shape == (8, 2) and fe._tables[0].shape == (3, 8, 2)
        meters = []
        for _ in range(7):
            fe.run()
            meters.append(st.meters())
        torch.cuda.synchronize()
        assert st.steps_done == 7 and fe._epoch == 2 and fe._pos == 2
        out.append((s._flat.clone(), t._flat.clone(), meters, {e: v.copy() for e, v in fe.host_tables.items()}))
        st.close()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and all(np.isfinite(m["loss"]) for m in out[0][2])
    np.random.seed(2024)
    want = [ws.epoch_table(e) for e in range(4)]
    for run in out:
        assert sorted(run[3]) == [2, 3] and all(np.array_equal(run[3][e], want[e]) for e in (2, 3))
    assert not np.array_equal(want[0][..., 1], want[1][..., 1]) and (want[0][:, 6:, 0] >= 20).all()


def test_windowed_feeding_equals_host_feeding():
    """The same windows (the epoch tables under the same numpy seed) cut on the host, transformed by LogMelTransform with the
    front-end's key sequence and fed through step.step, give a bit-identical student; feeding each batch the previous batch's
    targets does not.  Every window is full, so the dense batch's noise stride is the gather's."""
    from dcase2019_task4_amd.features import LogMelTransform
    from dcase2019_task4_amd.resident import ResidentFrontEnd
    ws = _train_set(full=True)
    feats, labels, sc = _train_items(True)
    n = 7
    np.random.seed(77)
    st, s_res, _ = _mt_step(ws)
    fe = ResidentFrontEnd(st, ws)
    for _ in range(n):
        fe.run()
    torch.cuda.synchronize()
    st.close()
    np.random.seed(77)
    rows = np.concatenate([ws.epoch_table(e) for e in range(3)])[:n]
    assert rows[:, 6:, 1].max() > 0                                  # crops inside the recordings are in play
    keys = _keys(ws.seed, n)
    tr = LogMelTransform(T, sc, augment_type="noise")
    cut = [[wn.cut_window(feats[i], labels[i], s3, T, P8) for i, s3 in row] for row in rows]
    assert all(c[0].shape[0] == T for row in cut for c in row)
    xs = [torch.tensor(np.stack([c[0] for c in row])).cuda() for row in cut]
    gs = [torch.tensor(np.stack([c[1] for c in row])).cuda() for row in cut]

    def host(lag):
        st, s, _ = _mt_step(ws)
        for k in range(n):
            x, x_ema = tr(xs[k], seed=keys[k])
            st.step(x, x_ema, gs[max(0, k - lag)])
        torch.cuda.synchronize()
        st.close()
        return s._flat.clone()

    assert torch.equal(s_res._flat, host(0))
    assert not torch.equal(s_res._flat, host(1))


def test_windowed_front_end_with_a_policy_augments_the_staged_windows():
    """With an AugmentPolicy the slot the front-end fills equals the numpy statement of the augmentation applied to the window
    gather of the staged row, bit for bit - at start-up and one batch ahead."""
    from dcase2019_task4_amd.augment import AugmentPolicy
    from dcase2019_task4_amd.resident import ResidentFrontEnd
    pol = AugmentPolicy(mixup_alpha=0.4, mixup_prob=0.8, shift_std=6.0, freq_mask_max=10, time_mask_max=12, seed=31)
    ws = _train_set(augment=pol)
    np.random.seed(4)
    st, _, _ = _mt_step(ws)
    fe = ResidentFrontEnd(st, ws)
    assert fe.aug
    keys = _keys(ws.seed, 2)
    fe.prime()
    fe.run()
    torch.cuda.synchronize()
    assert (fe.host_aug_tables[0][:2, :, 0] != np.arange(8)).any()                   # mixup is live in these rows
    for k, slot in ((0, fe._slots[0]), (1, fe._slots[1])):
        x, xe, g = ws.transform(fe.host_tables[0][k], seed=keys[k])
        table = fe.host_aug_tables[0][k]
        want = augment_np.augment(x.cpu().numpy(), xe.cpu().numpy(), g.cpu().numpy(), table)
        for got, w in zip(slot, want):
            assert np.array_equal(got.cpu().numpy().reshape(w.shape).view(np.uint32), w.view(np.uint32))
    st.close()


def test_train_with_a_windowed_set():
    from dcase2019_task4_amd.train import train
    ws = _train_set()
    student, _ = gu.make_model(0, dropout=0.5)
    teacher, _ = gu.make_model(1, dropout=0.5)
    opt = torch.optim.Adam(student.parameters(), lr=1e-3, betas=(0.9, 0.999))
    lines = []
    np.random.seed(5)
    ms = [train(ws, student, opt, e, ema_model=teacher, weak_mask=ws.weak_mask, strong_mask=ws.strong_mask, log=lines.append)
          for e in range(2)]
    st, fe = student._mt_step, student._mt_frontend
    assert st.steps_done == 2 * ws.n_steps == 6 and st.read_state().global_step == 6
    assert all(np.isfinite(v) for m in ms for v in m.values()) and lines[1].startswith("Epoch: 1\tTime ")
    np.random.seed(5)
    want = [ws.epoch_table(e) for e in range(4)]
    assert not np.array_equal(want[0][..., 1], want[1][..., 1])                      # fresh crops in the second epoch
    # (six steps staged seven batches: epoch 2's first, which drew epoch 3's table; the two live tables are kept)
    assert sorted(fe.host_tables) == [2, 3] and all(np.array_equal(fe.host_tables[e], want[e]) for e in (2, 3))
    st.close()


def test_a_plain_resident_set_keeps_its_front_end():
    """The front-end of a plain ResidentFeatureSet holds the tensors it held before windows existed - the key, the [B] index
    row, the workspace, two [n_steps, B] tables and the second slot - so the graph it captures has nothing new to read."""
    from dcase2019_task4_amd.resident import ResidentFeatureSet, ResidentFrontEnd
    feats, labels, sc = _train_items(False)
    rs = ResidentFeatureSet.from_arrays(feats[:20], labels[:20], (8, 8, 4), BSZ, frames=T, scaler=sc, seed=5)
    st, _, _ = _mt_step(rs)
    fe = ResidentFrontEnd(st, rs)
    tensors = {k: v for k, v in vars(fe).items() if torch.is_tensor(v)}
    assert sorted(tensors) == ["idx", "key", "ws_t"]
    assert fe.idx.shape == (st.B,) and fe.idx.dtype == torch.int32
    assert [tuple(t.shape) for t in fe._tables] == [(2, st.B)] * 2 and not fe.aug
    assert len(fe._slots) == 2 and fe._slots[0][0] is st.x
    st.close()

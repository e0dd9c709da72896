"""-m gpu: the feature front-end (csrc/feat.hip) off its 64-band, even-sized default path, against the numpy oracle - the
STFT at clips shorter than one window, at the fast path's exact edges and at degenerate frame counts; the log-mel chain at
odd element counts (where k_logmel_max shifts its Philox pairs), tiny clips, 40 / 65 / 128 bands and placed top-dB clamps;
the merged and the window gather at odd noise strides; the scaler statistics at every column count the divisor rule admits.
What each shape exercises is stated in tests/frontend_shapes.py and proved without a GPU in tests/test_frontend_shapes_cpu.py.
Bounds are the project's own (tests/test_gpu_features.py, tests/test_gpu_resident.py)."""
import types

import numpy as np
import pytest
import torch

from oracle import features_np, philox
from tests import frontend_shapes as fs
from tests import window_np as wn

pytestmark = pytest.mark.gpu

DB_ATOL = 2e-5                 # f64 mode against the oracle (dB, or units of the per-band std with a scaler)
F32_DB, F32_NORM = 1e-3, 2e-4  # f32 mode against the f64 mode: dB without a scaler, units of the per-band std with one
_WANT = {}


def _want_mel(case, n_mels):
    """The oracle's linear mel of every clip of a case, computed once."""
    if (case, n_mels) not in _WANT:
        waves = fs.stft_waves(case)
        _WANT[case, n_mels] = waves, [fs.mel_oracle(w, case[2], n_mels) for w in waves]
    return _WANT[case, n_mels]


def _extractor(hop, n_mels):
    from dcase2019_task4_amd.features import FeatureConfig, FeatureExtractor
    return FeatureExtractor(FeatureConfig(sample_rate=16000, n_window=2048, hop_length=hop, n_mels=n_mels, f_min=0.0, f_max=8000.0))


def _check_mel(got, want, mode, what):
    worst = 0.0
    for g, w in zip(got, want):
        worst = max(worst, np.abs(g - w).max() / w.max())
    bound = "rtol 2e-6 + 1e-6 of max" if mode == "f64" else "3e-6 of max"
    print(f"[frontend shapes] {what} {mode}: max err {worst:.2e} of the clip maximum (bound {bound})")
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.isfinite(g).all()
        if mode == "f64":
            np.testing.assert_allclose(g, w, rtol=fs.MEL_RTOL, atol=fs.MEL_ATOL_OF_MAX * w.max())
        else:
            assert np.abs(g - w).max() < fs.MEL_F32_OF_MAX * w.max()


# ---- 1. STFT + mel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,n_mels", fs.STFT_RUNS, ids=str)
def test_mel_frames_vs_oracle_at_short_clips_and_path_edges(case, n_mels):
    """sed_mel_frames against features_np.calculate_mel_spec, fp64 and f32 mode; 1, 3 and the default number of workgroups
    give the same bytes."""
    n_clips, n_samples, hop = case
    fe = _extractor(hop, n_mels)
    waves, want = _want_mel(case, n_mels)
    g = fs.stft_geometry(n_samples, hop)
    x = torch.tensor(waves).cuda()
    for mode in ("f64", "f32"):
        ref = fe.calculate_mel_spec_batch(x, fft_dtype=mode)
        assert ref.shape == (n_clips, g["frames"], n_mels)
        for wgs in (1, 3):
            assert torch.equal(fe.calculate_mel_spec_batch(x, workgroups=wgs, fft_dtype=mode), ref), (mode, wgs)
        _check_mel(ref.cpu().numpy(), want, mode,
                   f"stft {case} x {n_mels} bands (both-ends {g['both']}, base0 {g['base0']}, end {g['end']})")


@pytest.mark.parametrize("case", fs.STFT_OLD_KERNEL_CASES, ids=str)
def test_the_two_older_stft_kernels_vs_oracle_at_short_clips(case):
    """The wave-per-frame and the workgroup-per-frame kernel behind their debug bits reflect with code of their own: held to
    the oracle, not only to the persistent kernel."""
    from dcase2019_task4_amd import _lib
    fe = _extractor(case[2], 64)
    waves, want = _want_mel(case, 64)
    x = torch.tensor(waves).cuda()
    l = _lib.lib()
    got = {}
    try:
        for bit in (1 << 21, 1 << 19):
            l.sed_debug_set(bit)
            got[bit] = fe.calculate_mel_spec_batch(x)
            torch.cuda.synchronize()
    finally:
        l.sed_debug_set(0)
    for bit, m in got.items():
        _check_mel(m.cpu().numpy(), want, "f64", f"stft {case} older kernel (debug bit {bit.bit_length() - 1})")


# ---- 2. the dense transform ---------------------------------------------------------------------------------------------------
def _poisoned(*shape):
    return torch.full(shape, -1, device="cuda", dtype=torch.int32).view(torch.float32)          # NaN bytes


def _dense(mel, max_frames, scaler, seed, math_dtype):
    """sed_logmel_transform called directly, into buffers that start as NaN bytes -> (clean, noisy or None) on the host."""
    from dcase2019_task4_amd import _lib
    l = _lib.lib()
    x = torch.tensor(mel).cuda().contiguous()
    n, frames, n_mels = x.shape
    clean = _poisoned(n, 1, max_frames, n_mels)
    noisy = _poisoned(n, 1, max_frames, n_mels) if seed is not None else None
    key = torch.tensor([seed], dtype=torch.int64, device="cuda") if seed is not None else None
    mean = std = None
    if scaler is not None:
        mean = torch.tensor(np.asarray(scaler.mean_), dtype=torch.float64, device="cuda")
        std = torch.tensor(np.asarray(scaler.std_), dtype=torch.float64, device="cuda")
    ws = _poisoned(l.sed_logmel_transform_ws_bytes(n) // 4)
    _lib.check(l.sed_logmel_transform(_lib.ptr(x), n, frames, n_mels, max_frames, _lib.ptr(mean), _lib.ptr(std), _lib.ptr(key),
                                      _lib.ptr(clean), _lib.ptr(noisy), _lib.ptr(ws), ws.numel() * 4, _lib.FFT_DTYPES[math_dtype],
                                      _lib.stream_ptr()), "sed_logmel_transform")
    torch.cuda.synchronize()
    return clean.cpu().numpy(), None if noisy is None else noisy.cpu().numpy()


def _own_scaler(mel, max_frames):
    """Scaler statistics of the inputs themselves, through the oracle's chain (as test_logmel_transform_vs_oracle)."""
    with np.errstate(invalid="ignore"):
        mean, _, std = features_np.scaler_stats([features_np.transform_chain(m, max_frames) for m in mel])
    return types.SimpleNamespace(mean_=mean, std_=std)


def _max_err(a, b):
    """max |a - b| where both are numbers; NaN must sit at the same elements of both (a band without variance)."""
    assert np.array_equal(np.isnan(a), np.isnan(b))
    d = np.abs(a - b)[~np.isnan(a)]
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize("with_scaler", [False, True], ids=["db", "scaled"])
@pytest.mark.parametrize("case", fs.DENSE_CASES, ids=str)
def test_logmel_transform_vs_oracle_at_odd_and_small_sizes(case, with_scaler):
    """noise -> dB (top-dB clamp over the whole clip) -> pad / truncate -> normalise against transform_chain with
    philox.teacher_noise, with and without noise, f64 mode at 2e-5 and f32 mode against it at 1e-3 dB / 2e-4 of the std.
    The scaler is the inputs' own; the one-element case has no variance, its reference output is NaN and so must the
    kernel's be (tests/test_frontend_shapes_cpu.py)."""
    n, frames, n_mels, max_frames = case
    mel = fs.dense_mel(case)
    sc = _own_scaler(mel, max_frames) if with_scaler else None
    ms = (sc.mean_, sc.std_) if with_scaler else (None, None)
    seed = 987654321 + n_mels
    noise = philox.teacher_noise(seed, n, frames, n_mels).astype(np.float64)
    want_c = np.stack([features_np.transform_chain(mel[i], max_frames, *ms) for i in range(n)])
    with np.errstate(invalid="ignore"):
        want_n = np.stack([features_np.transform_chain(mel[i], max_frames, *ms, noise[i])[1] for i in range(n)])
    finite = not with_scaler or bool(np.isfinite(sc.std_).all())
    assert finite == (not with_scaler or case != (1, 1, 1, 1)) and np.isfinite(want_c).all() == finite
    res = {}
    for md in ("f64", "f32"):
        clean, noisy = _dense(mel, max_frames, sc, seed, md)
        only_clean, none = _dense(mel, max_frames, sc, None, md)
        assert none is None and np.array_equal(only_clean, clean, equal_nan=True)       # the clean copy ignores the noise
        assert clean.shape == noisy.shape == (n, 1, max_frames, n_mels)
        res[md] = clean, noisy
    c, z = res["f64"]
    ec, en = _max_err(c, want_c), _max_err(z, want_n)
    fc, fn = _max_err(res["f32"][0], c), _max_err(res["f32"][1], z)
    f32_bound = F32_NORM if with_scaler else F32_DB
    print(f"[frontend shapes] dense {case} {'scaled' if with_scaler else 'db'}: f64 clean {ec:.2e} noisy {en:.2e} (bound {DB_ATOL:.0e}); "
          f"f32 vs f64 clean {fc:.2e} noisy {fn:.2e} (bound {f32_bound:.0e})")
    np.testing.assert_allclose(c, want_c, rtol=0, atol=DB_ATOL)
    np.testing.assert_allclose(z, want_n, rtol=0, atol=DB_ATOL)
    assert fc < f32_bound and fn < f32_bound
    if not with_scaler and max_frames > frames:                 # pad rows: exactly 0 dB, in every mode
        for md in res:
            for out in res[md]:
                assert (out[:, :, frames:] == 0.0).all() and (out[:, :, :frames] != 0.0).any()
    if finite:
        assert all(np.isfinite(o).all() for md in res for o in res[md])
        assert not np.array_equal(c, z)


def test_some_dense_case_draws_from_an_odd_noise_base():
    assert any((c * frames * n_mels) % 2 == 1 for n, frames, n_mels, _ in fs.DENSE_CASES for c in range(n))


# ---- 3. clamp placement -------------------------------------------------------------------------------------------------------
def _clamp_check(mel, max_frames, seed, what):
    """f64 mode against the oracle, clean and noisy, no scaler -> the f64 outputs."""
    n, frames, n_mels = mel.shape
    noise = philox.teacher_noise(seed, n, frames, n_mels).astype(np.float64)
    want = [features_np.transform_chain(mel[i], max_frames, noise=noise[i]) for i in range(n)]
    want_c, want_n = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    c, z = _dense(mel, max_frames, None, seed, "f64")
    print(f"[frontend shapes] clamp {what}: f64 clean {_max_err(c, want_c):.2e} noisy {_max_err(z, want_n):.2e} (bound {DB_ATOL:.0e})")
    np.testing.assert_allclose(c, want_c, rtol=0, atol=DB_ATOL)
    np.testing.assert_allclose(z, want_n, rtol=0, atol=DB_ATOL)
    return c, z, want_c


def test_top_db_floor_comes_from_the_whole_clip_when_the_peak_is_truncated():
    """9 frames of 5 bands, 4 kept; frame 6 - dropped by the truncation - is 60 dB above the rest, and kept frame 1 is 60 dB
    below it.  The floor is the dropped peak's - 80 dB, so frame 1 is clamped 20 dB up; a floor taken from the kept frames
    alone would leave it where it is."""
    rs = np.random.RandomState(3)
    mel = (np.abs(rs.standard_normal((2, 9, 5))) + 0.5).astype(np.float32)
    mel[:, 6] *= 1e3
    mel[:, 1] *= 1e-3
    c, _, want_c = _clamp_check(mel, 4, 424242, "truncated peak")
    peak_db = 20 * np.log10(mel.max(axis=(1, 2)))
    for i in range(2):
        assert np.allclose(c[i, 0, 1], peak_db[i] - 80.0, atol=1e-4)                              # clamped to the whole clip's floor
        kept_only = features_np.transform_chain(mel[i, :4], 4)
        assert (kept_only[0, 1] < c[i, 0, 1] - 15.0).all()                                        # ... which the kept frames do not set
    # f32 mode: the same clamp
    c32, _ = _dense(mel, 4, None, 424242, "f32")
    assert _max_err(c32, c) < F32_DB


@pytest.mark.parametrize("level,what", [(0.0, "silent"), (1e-7, "sub-amin")])
def test_clips_at_or_below_amin(level, what):
    """A clip of zeros and a clip wholly below amin = 1e-5 (beside an ordinary one: the clamp is per clip), padded by a frame.
    Clean: -100 dB everywhere, 0 dB in the pad row.  Noisy, f64 mode: the oracle's.
    f32 mode: only the clean output is held to the f64 mode.  The mode's bounds (1e-3 dB) are stated for clips whose level
    dominates the noise.  Here the noise ALONE sets the level, and the fp32 Box-Muller draw (u1 and u2 on a 2^-24 grid once
    they are float32) differs from the fp64 one by far more than 1e-3 dB for small draws: |N| near 0 comes from cos / sin
    near a zero, where an absolute 2^-24 in u2 is a large relative change.  That is the mode's arithmetic, not a kernel error,
    so the noisy output is asserted finite and not below its own floor."""
    frames, n_mels, max_frames = 3, 5, 4
    mel = fs.dense_mel((2, frames, n_mels, max_frames), seed=7)
    mel[0] = level
    c, z, _ = _clamp_check(mel, max_frames, 1357911, what)
    assert (c[0, 0, :frames] == -100.0).all() and (c[0, 0, frames:] == 0.0).all() and (c[1, 0, :frames] > -50.0).all()
    assert z[0, 0, :frames].max() > -60.0 and (z[0, 0, :frames] >= z[0, 0, :frames].max() - 80.0 - 1e-4).all()
    c32, z32 = _dense(mel, max_frames, None, 1357911, "f32")
    assert _max_err(c32, c) < F32_DB
    assert np.isfinite(z32).all() and (z32[:, 0, frames:] == 0.0).all()
    for i in range(2):
        assert (z32[i, 0, :frames] >= z32[i, 0, :frames].max() - 80.0 - F32_DB).all()
    assert _max_err(z32[1], z[1]) < F32_DB                                                        # the ordinary clip beside it keeps the bound


# ---- 4. the gathers at odd strides --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", fs.GATHER_BANDS)
def test_gather_transform_vs_oracle_at_odd_noise_strides(n_mels):
    """A ragged pool of 5 bands (L_max * n_mels = 65: every odd batch position draws from an odd counter), gathered with
    repeats and out of order: features against transform_chain with the noise teacher_noise(seed, B, L_max, n_mels)[b, :len],
    targets exact.  The same with 40 and 128 bands (even strides)."""
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    T, lengths, idx = fs.GATHER_FRAMES, fs.GATHER_LENGTHS, fs.GATHER_IDX
    feats = fs.gather_clips(n_mels)
    feats[3][2, :] *= 1e-7                                       # the amin floor / the top-dB clamp
    tgts = [np.random.RandomState(50 + i).uniform(-1, 1, size=(3, 7)).astype(np.float32) for i in range(len(lengths))]
    sc = _own_scaler(feats[:4], T)
    assert np.isfinite(sc.std_).all()
    seed = 987654321
    noise = philox.teacher_noise(seed, len(idx), max(lengths), n_mels)
    res = {}
    for md in ("f64", "f32"):
        rs = ResidentFeatureSet.from_arrays(feats, tgts, frames=T, scaler=sc, math_dtype=md)
        clean, noisy, tgt = rs.transform(idx, seed=seed)
        assert clean.shape == noisy.shape == (len(idx), 1, T, n_mels) and tgt.shape == (len(idx), 3, 7)
        np.testing.assert_array_equal(tgt.cpu().numpy(), np.stack([tgts[i] for i in idx]))
        res[md] = clean.cpu().numpy(), noisy.cpu().numpy()
    c, z = res["f64"]
    ec = en = 0.0
    want = [features_np.transform_chain(feats[i], T, sc.mean_, sc.std_, noise[b, :lengths[i]].astype(np.float64))
            for b, i in enumerate(idx)]
    for b, (wc, wz) in enumerate(want):
        ec, en = max(ec, np.abs(c[b] - wc).max()), max(en, np.abs(z[b] - wz).max())
    fc, fn = np.abs(res["f32"][0] - c).max(), np.abs(res["f32"][1] - z).max()
    print(f"[frontend shapes] gather {n_mels} bands: f64 clean {ec:.2e} noisy {en:.2e} (bound {DB_ATOL:.0e}); "
          f"f32 vs f64 clean {fc:.2e} noisy {fn:.2e} (bound {F32_NORM:.0e})")
    for b, (wc, wz) in enumerate(want):
        np.testing.assert_allclose(c[b], wc, rtol=0, atol=DB_ATOL, err_msg=f"position {b}")
        np.testing.assert_allclose(z[b], wz, rtol=0, atol=DB_ATOL, err_msg=f"position {b}")
    assert fc < F32_NORM and fn < F32_NORM
    # repeated clips at positions of different parity: same clean bytes, different noise
    assert np.array_equal(c[0], c[3]) and not np.array_equal(z[0], z[3]) and np.array_equal(c[5], c[6])


@pytest.mark.parametrize("T", [8, 11], ids=["truncated", "padded"])
@pytest.mark.parametrize("math_dtype", ["f64", "f32"])
def test_gather_equal_length_odd_sized_pool_is_bit_identical_to_logmel_transform(math_dtype, T):
    """An equal-length pool of (9 frames, 5 bands): the gather's noise stride is the dense batch's 45, odd."""
    from dcase2019_task4_amd.features import LogMelTransform
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    feats = fs.gather_clips(5, lengths=[9] * 6, seed=3)
    sc = _own_scaler(feats[:4], T)
    idx = [4, 1, 1, 5, 0]
    stacked = torch.tensor(np.stack([feats[i] for i in idx])).cuda()
    seed = 0x5EADBEEF12345678
    rs = ResidentFeatureSet.from_arrays(feats, None, frames=T, scaler=sc, math_dtype=math_dtype)
    clean, noisy, tgt = rs.transform(idx, seed=seed)
    assert tgt is None and clean.shape == (5, 1, T, 5)
    wc, wn = LogMelTransform(T, sc, augment_type="noise", math_dtype=math_dtype)(stacked, seed=seed)
    assert torch.equal(clean, wc) and torch.equal(noisy, wn) and not torch.equal(noisy, clean)
    ev = ResidentFeatureSet.from_arrays(feats, None, frames=T, scaler=sc, augment_type=None, math_dtype=math_dtype)
    (vc, _) = ev.transform(idx)
    assert torch.equal(vc, LogMelTransform(T, sc, math_dtype=math_dtype)(stacked)) and torch.equal(vc, clean)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("math_dtype", ["f64", "f32"])
def test_window_gather_at_an_odd_noise_stride_is_bit_identical_to_the_merged_gather(math_dtype):
    """33-frame windows of 5 bands at pooling ratio 4 (max_win_frames * n_mels = 165): the window gather against the merged
    gather on the same windows cut on the host, and the f64 mode against the oracle."""
    from dcase2019_task4_amd.longrec import WindowedFeatureSet
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    F, P, n_mels, nclass = fs.WINDOW_FRAMES, fs.WINDOW_POOL, fs.WINDOW_BANDS, 3
    lengths = [1, 31, 33, 34, 100, 259]
    windows = [(5, 0), (5, 56), (4, 17), (5, 30), (0, 0), (4, 3), (1, 0), (1, 7), (5, 64), (2, 0), (3, 0), (3, 8), (4, 0)]
    rs_ = np.random.RandomState(0)
    feats = [(np.abs(rs_.standard_normal((n, n_mels))) * 3.0).astype(np.float32) for n in lengths]
    feats[4][20:70] *= 1e-7
    labels = [rs_.uniform(-1, 1, size=(max(1, n // P), nclass)).astype(np.float32) for n in lengths]
    sc = types.SimpleNamespace(mean_=rs_.uniform(-30, -10, n_mels), std_=rs_.uniform(5, 15, n_mels))
    kw = dict(scaler=sc, augment_type="noise", math_dtype=math_dtype)
    ws = WindowedFeatureSet.from_arrays(feats, labels, [3, 3], [1, 1], F, [False, True], pooling_time_ratio=P, **kw)
    cuts = [wn.cut_window(feats[i], labels[i], s, F, P) for i, s in windows]
    assert max(c[0].shape[0] for c in cuts) == F == ws.max_win_frames and min(c[0].shape[0] for c in cuts) == 1
    plain = ResidentFeatureSet.from_arrays([c[0] for c in cuts], [c[1] for c in cuts], frames=F, **kw)
    seed = 0x1234567
    got = ws.transform(windows, seed=seed)
    want = plain.transform(np.arange(len(windows)), seed=seed)
    for g, w in zip(got, want):
        assert torch.equal(_bits(g), _bits(w)) and torch.isfinite(g).all()
    np.testing.assert_array_equal(got[2].cpu().numpy(), np.stack([c[1] for c in cuts]))
    assert not torch.equal(got[0], got[1])
    if math_dtype == "f64":
        noise = philox.teacher_noise(seed, len(windows), F, n_mels)
        for b, (f, _) in enumerate(cuts):
            wc, wz = features_np.transform_chain(f, F, sc.mean_, sc.std_, noise[b, :f.shape[0]].astype(np.float64))
            np.testing.assert_allclose(got[0][b].cpu().numpy(), wc, rtol=0, atol=DB_ATOL)
            np.testing.assert_allclose(got[1][b].cpu().numpy(), wz, rtol=0, atol=DB_ATOL)


# ---- 5. scaler statistics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cols", fs.SCALER_COLS)
def test_scaler_stats_at_every_column_count_and_ragged_row_counts(n_cols):
    """sed_scaler_stats against a float64 numpy column sum; a second call adds to the sums it finds."""
    from dcase2019_task4_amd import _lib
    l = _lib.lib()
    for rows in fs.scaler_rows(n_cols):
        x = (np.random.RandomState(rows + n_cols).standard_normal((rows, n_cols)) * 8.0 - 20.0).astype(np.float32)
        xd = torch.tensor(x).cuda()
        sums = torch.zeros(2 * n_cols, dtype=torch.float64, device="cuda")
        _lib.check(l.sed_scaler_stats(_lib.ptr(xd), rows, n_cols, _lib.ptr(sums), _lib.stream_ptr()), "sed_scaler_stats")
        once = sums.cpu().numpy()
        _lib.check(l.sed_scaler_stats(_lib.ptr(xd), rows, n_cols, _lib.ptr(sums), _lib.stream_ptr()), "sed_scaler_stats")
        twice = sums.cpu().numpy()
        x64 = x.astype(np.float64)
        want = np.concatenate([x64.sum(axis=0), (x64 * x64).sum(axis=0)])
        err = np.abs(once / want - 1.0).max()
        print(f"[frontend shapes] scaler stats {rows} rows x {n_cols} cols: max relative err {err:.2e} (bound 1e-06)")
        np.testing.assert_allclose(once, want, rtol=1e-6)
        np.testing.assert_allclose(twice, 2.0 * want, rtol=1e-6)


def test_scaler_device_pass_refuses_40_bands_and_touches_nothing():
    from dcase2019_task4_amd import _lib
    from dcase2019_task4_amd.features import Scaler
    l = _lib.lib()
    x = torch.tensor(fs.dense_mel((2, 33, 40, 40))).cuda()
    sc = Scaler()
    with pytest.raises(_lib.SedError, match="n_cols must divide 256"):
        sc.calculate_scaler_device([x])
    assert sc.mean_ is None and sc.mean_of_square_ is None and sc.std_ is None
    sums = torch.full((80,), 0.5, dtype=torch.float64, device="cuda")
    assert l.sed_scaler_stats(_lib.ptr(x), 66, 40, _lib.ptr(sums), _lib.stream_ptr()) != 0
    assert b"n_cols must divide 256" in l.sed_last_error()
    torch.cuda.synchronize()
    assert (sums == 0.5).all()

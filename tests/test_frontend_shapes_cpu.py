"""What the cases of tests/test_gpu_frontend_shapes.py claim to exercise, proved on the CPU (no GPU, no library): frame
geometry of every STFT case, what fp32 arithmetic alone costs at those shapes, which dense / gather cases draw their noise
from an odd counter, and that the oracle's noise is one stream whatever the shape."""
import numpy as np
import pytest

from oracle import features_np, philox
from tests import frontend_shapes as fs


@pytest.mark.parametrize("case", list(fs.STFT_CASES), ids=str)
def test_stft_case_exercises_what_it_claims(case):
    n_clips, n_samples, hop = case
    claim = fs.STFT_CASES[case]
    g = fs.stft_geometry(n_samples, hop)
    print(f"[frontend shapes] stft {case}: {g}")
    assert n_samples > fs.NFFT // 2                                    # the entry accepts it
    for key in ("both", "base0", "end", "fast"):
        if key in claim:
            assert claim[key] >= 1 and g[key] >= claim[key], (key, g)
    if "frames" in claim:
        assert g["frames"] == claim["frames"]
    if "total" in claim:
        assert n_clips * g["frames"] == claim["total"]
    if claim.get("odd_base"):
        assert n_clips >= 2 and (n_samples * 4) % 8 == 4               # clip 1 starts 4 bytes off an 8-byte boundary
    # reflection at both ends exists only for the lengths under one window, where no frame is free of reflection
    if n_samples < fs.NFFT:
        assert g["fast"] == 0
    else:
        assert g["both"] == 0


def test_stft_cases_as_a_set():
    g = {c: fs.stft_geometry(c[1], c[2]) for c in fs.STFT_CASES}
    # frame 4 of (2, 4096, 256) starts at sample 0 and frame 12 ends at the last sample; they are different frames
    base = 256 * np.arange(17) - 1024
    assert base[4] == 0 and base[12] + fs.NFFT == 4096
    # in (2, 2048, 512) one frame is the whole clip: both edges at once
    assert g[(2, 2048, 512)]["fast"] == 1 and 512 * 2 - 1024 == 0
    # a launch with fewer frames than a workgroup has waves; clips whose frames are no multiple of the waves, so that one
    # workgroup holds frames of two clips; a launch of more frames than one workgroup holds, run on one workgroup too
    assert 1 * g[(1, 1025, 2048)]["frames"] < fs.STP_WAVES
    assert g[(5, 2600, 64)]["frames"] % fs.STP_WAVES != 0 and 5 * g[(5, 2600, 64)]["frames"] > 3 * fs.STP_WAVES
    assert all(c in fs.STFT_CASES for c in fs.STFT_OLD_KERNEL_CASES)
    assert all(g[c]["both"] > 0 for c in fs.STFT_OLD_KERNEL_CASES[:2])
    assert all(c in fs.STFT_CASES for c, _ in fs.STFT_BAND_CASES)
    # at the default hop every length 1025 .. 2043 reflects a frame at both ends (frame 4 starts 4 samples before the
    # clip); none from 2048 on
    assert all(fs.stft_geometry(n, 255)["both"] > 0 for n in range(1025, 2044))
    assert all(fs.stft_geometry(n, 255)["both"] == 0 for n in (2048, 2500, 4096))


@pytest.mark.parametrize("case,n_mels", fs.STFT_RUNS, ids=str)
def test_float32_restatement_stays_within_a_quarter_of_each_bound(case, n_mels):
    """A float32 numpy / scipy restatement of calculate_mel_spec against the float64 oracle: what fp32 arithmetic alone costs
    at the shape.  It stays within a quarter of the fp64 mode's bound (rtol 2e-6, atol 1e-6 of the clip maximum) and of the
    f32 mode's (3e-6 of the clip maximum), so neither bound can be missed for the shape's sake."""
    _, _, hop = case
    waves = fs.stft_waves(case)
    worst = 0.0
    for w in waves:
        want = fs.mel_oracle(w, hop, n_mels)
        got = fs.mel_f32_restatement(w, hop, n_mels)
        assert got.shape == want.shape == (fs.stft_geometry(case[1], hop)["frames"], n_mels)
        err = np.abs(got - want)
        worst = max(worst, err.max() / want.max())
        assert (err <= 0.25 * (fs.MEL_ATOL_OF_MAX * want.max() + fs.MEL_RTOL * np.abs(want))).all()
        assert err.max() <= 0.25 * fs.MEL_F32_OF_MAX * want.max()
    print(f"[frontend shapes] stft {case} x {n_mels} bands: float32 restatement {worst:.2e} of the clip maximum")


def test_dense_cases_with_an_odd_noise_base():
    odd = {c: fs.odd_noise_clips(c[0], c[1] * c[2]) for c in fs.DENSE_CASES}
    assert {c: v for c, v in odd.items() if v} == fs.DENSE_ODD_BASE
    assert any((c * frames * n_mels) % 2 == 1 for n, frames, n_mels, _ in fs.DENSE_CASES for c in range(n))
    # an odd base needs an odd clip size: the cases with 40 and 128 bands have none, and say so
    assert odd[(2, 33, 40, 40)] == [] and odd[(3, 9, 128, 8)] == []
    # sizes around the LM_CHUNKS split: fewer elements than chunks, one element, and several 512-element strides per chunk
    assert 1 * 3 < fs.LM_CHUNKS and 627 * 65 == 40755 and 40755 // fs.LM_CHUNKS > 4 * 512
    # truncated, padded and exact
    assert {np.sign(mf - fr) for _, fr, _, mf in fs.DENSE_CASES} == {-1, 0, 1}


def test_the_one_element_case_has_no_statistics_of_its_own():
    """The scaler of every dense case is computed from the case's own inputs.  One value has no variance: up to the float32
    rounding of its square, E[x^2] - E[x]^2 is zero, and here it comes out negative, so the reference's Scaler yields
    std = NaN and the normalised output is NaN - which the kernel must reproduce element for element.  Every other case has
    a finite, non-zero standard deviation in every band."""
    for case in fs.DENSE_CASES:
        mel = fs.dense_mel(case)
        with np.errstate(invalid="ignore"):
            _, _, std = features_np.scaler_stats([features_np.transform_chain(m, case[3]) for m in mel])
        if case == (1, 1, 1, 1):
            assert np.isnan(std).all()
        else:
            assert np.isfinite(std).all() and std.min() > 1.0, (case, std.min())


def test_gather_cases_with_an_odd_noise_base():
    B, L_max = len(fs.GATHER_IDX), max(fs.GATHER_LENGTHS)
    assert L_max * 5 == 65 and fs.odd_noise_clips(B, L_max * 5) == [b for b in range(B) if b % 2 == 1]
    assert fs.odd_noise_clips(B, L_max * 40) == [] and fs.odd_noise_clips(B, L_max * 128) == []
    # repeats, out of order; the odd batch positions hold the one-frame clip and clips longer than the output
    idx = fs.GATHER_IDX
    assert len(set(idx)) < len(idx) and sorted(idx) != idx and set(idx) == set(range(len(fs.GATHER_LENGTHS)))
    at_odd = {np.sign(fs.GATHER_LENGTHS[idx[b]] - fs.GATHER_FRAMES) for b in range(1, B, 2)}
    assert at_odd == {-1, 1} and fs.GATHER_LENGTHS[idx[1]] == 1 and fs.GATHER_LENGTHS[idx[3]] == L_max
    # the window gather's stride
    assert (fs.WINDOW_FRAMES * fs.WINDOW_BANDS) % 2 == 1 and fs.WINDOW_FRAMES % fs.WINDOW_POOL != 0


def test_teacher_noise_is_one_stream_whatever_the_shape():
    """Element e of the flattened tensor draws from counter e alone: reshaping changes nothing, and a shorter tensor is a
    prefix of a longer one - also when the length is odd and the last pair is cut in half."""
    seed = 5
    flat = philox.teacher_noise(seed, 1, 1, 105).reshape(-1)
    assert np.array_equal(philox.teacher_noise(seed, 5, 3, 7).reshape(-1), flat)
    assert np.array_equal(philox.teacher_noise(seed, 3, 7, 5).reshape(-1), flat)
    assert np.array_equal(philox.teacher_noise(seed, 3, 5, 7).reshape(-1), flat)
    for n in (1, 2, 35, 64, 65, 104):
        assert np.array_equal(philox.teacher_noise(seed, 1, 1, n).reshape(-1), flat[:n]), n
    long = philox.teacher_noise(seed, 7, 13, 5).reshape(-1)
    assert np.array_equal(long[:105], flat) and not np.array_equal(long[105:210], flat)
    # so clip c of a batch with an odd stride S starts in the middle of a pair: its elements are flat[c S : (c + 1) S]
    assert np.array_equal(philox.teacher_noise(seed, 3, 7, 5)[1].reshape(-1), flat[35:70])
    assert flat.dtype == np.float32 and (flat >= 0).all() and len(np.unique(flat)) == 105
    assert not np.array_equal(philox.teacher_noise(seed + 1, 1, 1, 105).reshape(-1), flat)


def test_scaler_row_counts_cover_a_partial_pass():
    for n_cols in fs.SCALER_COLS:
        assert fs.SCALER_THREADS % n_cols == 0
        rpp = fs.SCALER_THREADS // n_cols
        rows = fs.scaler_rows(n_cols)
        assert rows[:2] == (1, 3) and rows[2] == rpp + 1 and rows[3] == 1000
        assert any(r % rpp for r in rows) or rpp == 1
    assert fs.SCALER_THREADS % 40 != 0                                 # 40 bands: refused by the divisor rule

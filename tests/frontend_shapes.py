"""The shapes the feature front-end (csrc/feat.hip) is pinned at off its 64-band, even-sized default path, and plain host
statements of what each of them exercises.  Shared by tests/test_frontend_shapes_cpu.py (which proves the claims on the CPU)
and tests/test_gpu_frontend_shapes.py (which runs the kernels at them), so that an edit of a shape cannot silently empty a
case: the claim beside it then fails without a GPU."""
import numpy as np

from oracle import features_np, synth

NFFT = 2048
STP_WAVES = 12                 # frames a workgroup of k_stft_mel_p holds at a time (one per wave)
LM_CHUNKS = 16                 # workgroups per clip of k_logmel_max
SCALER_THREADS = 256           # k_scaler_stats: rows_per_pass = 256 / n_cols

# fp64 mode: rtol 2e-6 + 1e-6 of the clip maximum; f32 mode: 3e-6 of the clip maximum (tests/test_gpu_features.py)
MEL_RTOL, MEL_ATOL_OF_MAX, MEL_F32_OF_MAX = 2e-6, 1e-6, 3e-6

# (n_clips, n_samples, hop) -> the least count of frames of ONE clip that the case claims
#   both    reflect at both ends (lengths 1025 .. 2047 only)
#   base0   start exactly at sample 0 (fast path, reads the first sample)
#   end     end exactly at the last sample (fast path, reads the last sample)
#   fast    take the fast path at all
# and, where the case is about them, the frames per clip and in the whole launch; odd_base: clip 1 starts 4 bytes off an
# 8-byte boundary (the fast path loads sample PAIRS)
STFT_CASES = {
    (1, 1025, 255): dict(both=4, frames=5),                    # the minimum length: frames 1-4 reflect at both ends
    (3, 1500, 255): dict(both=3),                              # frames 2-4 (6000-byte clips: bases stay 16-byte aligned)
    (2, 2047, 511): dict(frames=5, odd_base=True),             # odd length just under the window: no frame can go fast
    (2, 2048, 512): dict(base0=1, end=1, fast=1),              # a multiple of the hop: frame 2 is the whole clip
    (2, 4096, 256): dict(base0=1, end=1, fast=9),              # frame 4 starts at 0, frame 12 ends at n_samples
    (3, 4097, 256): dict(base0=1, fast=9, odd_base=True),      # odd clip stride
    (1, 1025, 2048): dict(frames=1, total=1),                  # one frame in the whole launch
    (2, 3000, 3001): dict(frames=1, total=2),                  # hop longer than the clip
    (5, 2600, 64): dict(frames=41, total=205),                 # a workgroup's waves cross clip boundaries
}
STFT_OLD_KERNEL_CASES = [(1, 1025, 255), (3, 1500, 255), (2, 4096, 256)]       # also run on the two older kernels
STFT_BAND_CASES = [((3, 1500, 255), 40), ((3, 1500, 255), 128)]                # 128: the path without an LDS table
STFT_RUNS = [(c, 64) for c in STFT_CASES] + STFT_BAND_CASES


def stft_geometry(n_samples, hop):
    """Per-clip frame counts of a clip of n_samples at this hop: frame k covers samples [k hop - 1024, k hop + 1024)."""
    frames = 1 + n_samples // hop
    base = hop * np.arange(frames) - NFFT // 2
    left, right = base < 0, base + NFFT > n_samples
    return dict(frames=frames, both=int((left & right).sum()), base0=int((base == 0).sum()),
                end=int((base + NFFT == n_samples).sum()), fast=int((~left & ~right).sum()))


def stft_waves(case):
    n_clips, n_samples, _hop = case
    return np.stack([synth.make_wave(30 + i, n_samples) for i in range(n_clips)]).astype(np.float32)


def mel_oracle(wave, hop, n_mels):
    return features_np.calculate_mel_spec(wave.astype(np.float64), 16000, NFFT, hop, n_mels, 0.0, 8000.0)


def mel_f32_restatement(wave, hop, n_mels):
    """calculate_mel_spec with every array float32: float32 window, scipy's float32 real FFT of float32 frames, float32
    filterbank product.  Its distance from the float64 oracle is what fp32 ARITHMETIC costs at a shape."""
    import scipy.fft
    win = features_np.hamming_window(NFFT).astype(np.float32)
    ypad = np.pad(np.asarray(wave, dtype=np.float32), NFFT // 2, mode="reflect")
    nf = 1 + (len(ypad) - NFFT) // hop
    idx = np.arange(NFFT)[None, :] + hop * np.arange(nf)[:, None]
    frames = ypad[idx] * win[None, :]
    assert frames.dtype == np.float32
    mag = np.abs(scipy.fft.rfft(frames, axis=1))
    assert mag.dtype == np.float32
    return mag @ features_np.mel_filterbank(16000, NFFT, n_mels, 0.0, 8000.0).T


# (n_clips, frames, n_mels, max_frames) of the dense transform
DENSE_CASES = [
    (3, 7, 5, 4),              # 35 elements per clip: clip 1's noise base is odd; truncated
    (3, 7, 5, 9),              # the same clip size, padded
    (1, 1, 1, 1),              # one element
    (2, 1, 3, 2),              # fewer elements than chunks
    (5, 15, 3, 15),            # 45 elements per clip
    (2, 33, 40, 40),           # 40 bands
    (3, 9, 128, 8),            # 128 bands
    (3, 627, 65, 628),         # 40 755 elements: odd, several 512-element strides per chunk
]
DENSE_ODD_BASE = {(3, 7, 5, 4): [1], (3, 7, 5, 9): [1], (2, 1, 3, 2): [1], (5, 15, 3, 15): [1, 3], (3, 627, 65, 628): [1]}


def odd_noise_clips(n_clips, stride):
    """Batch positions whose first noise counter c * stride is odd: k_logmel_max shifts its Philox pairs for those."""
    return [c for c in range(n_clips) if (c * stride) % 2 == 1]


def dense_mel(case, seed=11):
    n, frames, n_mels, _ = case
    return (np.abs(np.random.RandomState(seed).standard_normal((n, frames, n_mels))) * 3.0).astype(np.float32)


# the merged gather: ragged pool, repeats, out of order
GATHER_LENGTHS, GATHER_FRAMES, GATHER_IDX = [7, 1, 13, 9, 4], 8, [2, 1, 4, 2, 0, 3, 3]
GATHER_BANDS = [5, 40, 128]    # L_max * n_mels = 65 (every odd batch position has an odd noise base), 520, 1664


def gather_clips(n_mels, lengths=GATHER_LENGTHS, seed=11):
    rs = np.random.RandomState(seed + n_mels)
    return [(np.abs(rs.standard_normal((n, n_mels))) * 3.0).astype(np.float32) for n in lengths]


# the window gather at an odd noise stride: 33-frame windows of 5 bands (165), pooling ratio 4
WINDOW_FRAMES, WINDOW_POOL, WINDOW_BANDS = 33, 4, 5

SCALER_COLS = (1, 2, 8, 128, 256)


def scaler_rows(n_cols):
    """Row counts of sed_scaler_stats: one, fewer than a pass, one more than a pass, many passes with a ragged tail."""
    return (1, 3, SCALER_THREADS // n_cols + 1, 1000)

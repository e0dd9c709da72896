"""Train-time batch augmentation on the device: mixup of features and targets, a circular time shift of features and strong
targets, SpecAugment-style time / frequency masks (``sed_batch_augment``, csrc/augment.hip; the definitions are stated in
include/dcase_sed.h and are the project's own - the reference has no such code and no external package's parity is claimed).

* ``AugmentPolicy``: the host side.  ``draw`` produces one epoch of per-clip parameter rows
  ``{partner, lambda_bits, shift_x, shift_y, f0, fw, t0, tw}`` from a generator of its own - pure host code.
* ``augment_batch``: convenience for tests and tools - device tensors + a table -> new device tensors.
* ``resident.ResidentFeatureSet(..., augment=policy)`` holds a policy; ``resident.ResidentFrontEnd`` then runs the kernel
  inside its graph branch, behind the gather.

There is no CPU path for the augmentation itself."""
import numpy as np
import torch

from . import _lib

PARTNER, LAMBDA, SHIFT_X, SHIFT_Y, F0, FW, T0, TW = range(8)
_ONE_BITS = int(np.float32(1.0).view(np.int32))


def identity_table(*lead):
    """Rows that change nothing: partner = own position, lambda = 1, no shift, no mask; shape lead + (B, 8), B = lead[-1]."""
    t = np.zeros(tuple(lead) + (8,), dtype=np.int32)
    t[..., PARTNER] = np.arange(lead[-1], dtype=np.int32)
    t[..., LAMBDA] = _ONE_BITS
    return t


def validate_table(table, B):
    """A host table [..., B, 8] int32 -> the same, C-contiguous; raises SedError on a wrong shape / dtype or a partner outside
    [0, B) (the kernel clamps partners, so a bad table could never fault - it would silently mix the wrong clips)."""
    if not isinstance(table, np.ndarray) or table.dtype != np.int32:
        raise _lib.SedError(f"an augmentation table is an int32 numpy array, got {type(table).__name__}"
                            f"{' of ' + str(table.dtype) if isinstance(table, np.ndarray) else ''}")
    if table.ndim < 2 or table.shape[-2:] != (int(B), 8):
        raise _lib.SedError(f"augmentation table of shape {table.shape}, expected [..., {int(B)}, 8]")
    p = table[..., PARTNER]
    if p.size and (p.min() < 0 or p.max() >= B):
        raise _lib.SedError(f"augmentation table holds a partner outside [0, {int(B)})")
    return np.ascontiguousarray(table)


class AugmentPolicy:
    """Which augmentations a training set applies and how their per-clip parameters are drawn.

    ``mixup_alpha``: lambda ~ Beta(alpha, alpha) for a clip that mixes (None: no mixup); ``mixup_prob``: the probability
    that a clip mixes.  ``shift_std``: standard deviation, in LABEL frames, of the circular time shift: k = round(N(0, std)),
    shift_y = k, shift_x = k * (T // T3), so features and strong labels move together (None / 0: off; for T not a multiple
    of T // T3 - 628 against 78 label frames - the seam of the roll is inexact by the T - T3 * (T // T3) left-over frames).
    ``freq_mask_max`` / ``time_mask_max``: mask widths uniform in [0, max] (clipped to the tensor), at a uniform position
    (0: off).  The default policy has everything off and draws identity rows."""

    def __init__(self, mixup_alpha=None, mixup_prob=1.0, shift_std=None, freq_mask_max=0, time_mask_max=0, seed=0):
        if mixup_alpha is not None and not float(mixup_alpha) > 0.0:
            raise ValueError(f"mixup_alpha must be > 0 (or None), got {mixup_alpha}")
        if not 0.0 <= float(mixup_prob) <= 1.0:
            raise ValueError(f"mixup_prob must be in [0, 1], got {mixup_prob}")
        if shift_std is not None and float(shift_std) < 0.0:
            raise ValueError(f"shift_std must be >= 0 (or None), got {shift_std}")
        if int(freq_mask_max) < 0 or int(time_mask_max) < 0:
            raise ValueError("mask widths must be >= 0")
        self.mixup_alpha = None if mixup_alpha is None else float(mixup_alpha)
        self.mixup_prob = float(mixup_prob)
        self.shift_std = float(shift_std) if shift_std else None
        self.freq_mask_max = int(freq_mask_max)
        self.time_mask_max = int(time_mask_max)
        self.seed = int(seed)

    @property
    def active(self):
        return bool((self.mixup_alpha is not None and self.mixup_prob > 0.0) or self.shift_std or self.freq_mask_max
                    or self.time_mask_max)

    def draw(self, epoch, n_steps, stream_slices, T, T3, M, rank=0):
        """One epoch of parameter rows, int32 [n_steps, B, 8], B the end of the last slice.  ``stream_slices``: the slices of
        the (local) batch the streams occupy, in order; partners are drawn WITHIN a clip's own slice (weak with weak,
        unlabelled with unlabelled, strong with strong), so the loss masks keep their meaning.  The draws come from a
        generator of the policy's own, seeded from (seed, rank, epoch): numpy's global generator is never touched."""
        n_steps, T, T3, M = int(n_steps), int(T), int(T3), int(M)
        if n_steps < 1 or T < 1 or T3 < 1 or M < 1:
            raise ValueError(f"need n_steps, T, T3 and M >= 1, got {n_steps}, {T}, {T3}, {M}")
        bounds, at = [], 0
        for s in stream_slices:
            lo, hi = (s.start or 0, s.stop) if isinstance(s, slice) else (int(s[0]), int(s[1]))
            if lo != at or hi is None or hi < lo or (isinstance(s, slice) and s.step not in (None, 1)):
                raise ValueError(f"stream slices must tile the batch in order, got {list(stream_slices)}")
            bounds.append((lo, hi))
            at = hi
        B = at
        if B < 1:
            raise ValueError("an empty batch")
        mask64 = (1 << 64) - 1
        rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(
            [self.seed & mask64, int(rank) & mask64, int(epoch) & mask64])))
        tab = identity_table(n_steps, B)
        if self.mixup_alpha is not None and self.mixup_prob > 0.0:
            for lo, hi in bounds:
                n = hi - lo
                if n < 1:
                    continue
                mixes = rng.random((n_steps, n)) < self.mixup_prob
                lam = rng.beta(self.mixup_alpha, self.mixup_alpha, size=(n_steps, n)).astype(np.float32)
                partner = rng.integers(0, n, size=(n_steps, n)) + lo
                own = np.arange(lo, hi)[None, :]
                mixes &= (partner != own) & (lam != np.float32(1.0))           # such a clip does not mix: identity entries
                tab[:, lo:hi, PARTNER] = np.where(mixes, partner, own)
                tab[:, lo:hi, LAMBDA] = np.where(mixes, lam, np.float32(1.0)).astype(np.float32).view(np.int32)
        if self.shift_std:
            ratio = max(1, T // T3)
            kmax = (2 ** 31 - 1) // ratio
            k = np.clip(np.rint(rng.normal(0.0, self.shift_std, size=(n_steps, B))), -kmax, kmax).astype(np.int64)
            tab[..., SHIFT_Y] = k
            tab[..., SHIFT_X] = k * ratio
        for width_col, pos_col, wmax, n in ((FW, F0, self.freq_mask_max, M), (TW, T0, self.time_mask_max, T)):
            if wmax:
                w = rng.integers(0, min(wmax, n) + 1, size=(n_steps, B))
                tab[..., width_col] = w
                tab[..., pos_col] = rng.integers(0, n - w + 1)
        return validate_table(tab, B)


def augment_batch(x, x_ema, target, table):
    """Convenience (tests, tools): device tensors x [B, T, M] or [B, 1, T, M], x_ema (or None), target [B, T3, NC] (or None)
    and a table [B, 8] - a host int32 array (validated) or a device int32 tensor - -> (x', x_ema' or None, target' or None) as
    new tensors, by one sed_batch_augment launch on the current stream."""
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise _lib.SedError("augment_batch needs tensors on a GPU device (no CPU fallback)")
    if x.dtype != torch.float32 or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1):
        raise ValueError(f"x must be float32 [B, T, M] or [B, 1, T, M], got {x.dtype} {tuple(x.shape)}")
    B, T, M = x.shape[0], x.shape[-2], x.shape[-1]
    for name, t, shape in (("x_ema", x_ema, x.shape), ("target", target, None)):
        if t is None:
            continue
        if t.device != x.device or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor on {x.device}")
        if (shape is not None and t.shape != shape) or (shape is None and (t.dim() != 3 or t.shape[0] != B)):
            raise ValueError(f"{name} of shape {tuple(t.shape)} against x of {tuple(x.shape)}")
    if isinstance(table, torch.Tensor):
        if table.device != x.device or table.dtype != torch.int32 or table.shape != (B, 8):
            raise _lib.SedError(f"a device augmentation table is int32 [{B}, 8] on {x.device}")
        tab = table.contiguous()
    else:
        tab = validate_table(table, B)
        if tab.ndim != 2:
            raise _lib.SedError(f"augment_batch takes one batch's table [B, 8], got shape {tab.shape}")
        tab = torch.from_numpy(tab).to(x.device)
    x, x_ema, target = (None if t is None else t.contiguous() for t in (x, x_ema, target))
    out = [None if t is None else _lib.scratch(t.numel() * 4, t.device).view(torch.float32).view(t.shape) for t in (x, x_ema, target)]
    T3, NC = (target.shape[1], target.shape[2]) if target is not None else (0, 0)
    _lib.check(_lib.lib().sed_batch_augment(_lib.ptr(x), _lib.ptr(x_ema), _lib.ptr(target), _lib.ptr(tab), B, T, M, T3, NC,
                                            _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.stream_ptr()),
               "sed_batch_augment")
    return tuple(out)


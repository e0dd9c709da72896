"""TEST INFRASTRUCTURE ONLY - plain float64 statement of the CRNN's output heads (baseline/models/CRNN.py:74-81) and of the
mean-teacher loss with its gradient w.r.t. the student's posteriors (baseline/main.py:93-145, nn.BCELoss), in numpy and
without autograd.  Both functions take float32-VALUED arrays and compute in float64 from exactly those values.

BCELoss's two clamps, as torch states them: each logarithm is clamped at -100, and the gradient is
(p - t) / max((1 - p) p, float32(1e-12)).  A label group with lo == hi contributes 0 (include/dcase_sed.h: "lo==hi disables the term").
Independent of how the kernels tile the work."""
import numpy as np

ATT_MIN = float(np.float32(1e-7))      # the clamp of CRNN.py:80 as the float32 kernels hold it
GRAD_EPS = float(np.float32(1e-12))   # BCELoss's gradient clamp: torch holds it as a float32 constant in every dtype, as the kernels do
METERS = ("loss", "weak_class_loss", "strong_loss", "cons_strong", "cons_weak", "weak_ema_loss", "strong_ema_loss", "cons_weight")


def heads_forward(h, mask_scale, Wd, bd, Ws, bs):
    """h [B, T3, F] the GRU output as given, mask_scale the drop_rnn mask times its scale (or 1), dense / dense_softmax
    weights [NC, F] and biases [NC] -> strong [B, T3, NC], raw (the softmax BEFORE the clamp), att = clip(raw, 1e-7, 1),
    den [B, NC] = sum_t att, weak [B, NC] = sum_t strong att / den."""
    h, Wd, bd, Ws, bs = (np.asarray(a, dtype=np.float64) for a in (h, Wd, bd, Ws, bs))
    x = h * np.asarray(mask_scale, dtype=np.float64)
    B, T3, _ = x.shape
    NC = Wd.shape[0]
    strong, raw = np.empty((B, T3, NC)), np.empty((B, T3, NC))
    with np.errstate(over="ignore", under="ignore"):
        for b in range(B):
            for t in range(T3):
                zd = Wd @ x[b, t] + bd
                zs = Ws @ x[b, t] + bs
                strong[b, t] = 1.0 / (1.0 + np.exp(-zd))
                e = np.exp(zs - zs.max())
                raw[b, t] = e / e.sum()
    att = np.clip(raw, ATT_MIN, 1.0)
    den = att.sum(1)
    weak = (strong * att).sum(1) / den
    return strong, raw, att, den, weak


def pool(strong, att):
    """den, weak of given posteriors and attention (the last two lines of heads_forward)."""
    strong, att = np.asarray(strong, dtype=np.float64), np.asarray(att, dtype=np.float64)
    den = att.sum(1)
    return den, (strong * att).sum(1) / den


def _bce_sum(p, t):
    with np.errstate(divide="ignore"):
        lp, l1p = np.maximum(np.log(p), -100.0), np.maximum(np.log1p(-p), -100.0)
    return float(-(t * lp + (1.0 - t) * l1p).sum())


def _bce_grad(p, t):
    return (p - t) / np.maximum((1.0 - p) * p, GRAD_EPS)


def mt_loss(strong, weak, strong_ema, weak_ema, target, wlo, whi, slo, shi, cw):
    """-> (meters [8] in the order of METERS, d_strong [B, T3, NC], d_weak [B, NC]): rows [wlo, whi) carry weak labels
    (target.max over the frames), rows [slo, shi) strong labels; both consistency terms run over every row."""
    strong, weak, strong_ema, weak_ema, target = (np.asarray(a, dtype=np.float64) for a in (strong, weak, strong_ema, weak_ema, target))
    B, T3, NC = strong.shape
    cw = float(cw)
    m = np.zeros(8)
    d_strong = cw * 2.0 * (strong - strong_ema) / (B * T3 * NC)
    d_weak = cw * 2.0 * (weak - weak_ema) / (B * NC)
    if whi > wlo:
        n = (whi - wlo) * NC
        tw = target[wlo:whi].max(1)
        m[1] = _bce_sum(weak[wlo:whi], tw) / n
        m[5] = _bce_sum(weak_ema[wlo:whi], tw) / n
        d_weak[wlo:whi] += _bce_grad(weak[wlo:whi], tw) / n
    if shi > slo:
        n = (shi - slo) * T3 * NC
        ts = target[slo:shi]
        m[2] = _bce_sum(strong[slo:shi], ts) / n
        m[6] = _bce_sum(strong_ema[slo:shi], ts) / n
        d_strong[slo:shi] += _bce_grad(strong[slo:shi], ts) / n
    m[3] = cw * ((strong - strong_ema) ** 2).mean()
    m[4] = cw * ((weak - weak_ema) ** 2).mean()
    m[0] = m[1] + m[2] + m[3] + m[4]
    m[7] = cw
    return m, d_strong, d_weak

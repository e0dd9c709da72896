"""Helpers shared by the -m gpu parity tests: build the HIP module with procedural weights, build the
oracle's inputs (incl. the Philox dropout masks for a given seed) and compare."""
import numpy as np
import torch

from oracle import philox, ref_cpu, synth

CRNN_KW = dict(n_in_channel=1, nclass=10, attention=True, n_RNN_cell=64, n_layers_RNN=2, activation="glu", dropout=0.5,
               kernel_size=3 * [3], padding=3 * [1], stride=3 * [1], nb_filters=[64, 64, 64],
               pooling=list(3 * ((2, 4),)))


def make_model(seed=0, dropout=0.5, device="cuda", n_layers=2, nclass=10, C=64, H=64, mfma_dtype="f32"):
    from dcase2019_task4_amd.crnn import CRNN
    kw = dict(CRNN_KW, dropout=dropout, n_layers_RNN=n_layers, nclass=nclass, nb_filters=[C] * 3, n_RNN_cell=H,
              mfma_dtype=mfma_dtype)
    m = CRNN(**kw)
    params = synth.make_params(seed, n_layers_RNN=n_layers, nclass=nclass, nb_filters=(C,) * 3, n_RNN_cell=H)
    with torch.no_grad():
        for (n, p) in m.named_parameters():
            p.copy_(params[n])
    return m.to(device), params


HEAD_NAMES = ("dense.weight", "dense.bias", "dense_softmax.weight", "dense_softmax.bias")
# the ladder's biases: sigmoid logits from exact 0 (-120) through posteriors below the 1e-12 gradient clamp (-40, -30) to exact 1
# (30, 120), none in -88 .. -104 (include/dcase_sed.h: sigmoidf_fast); attention logits from the dominant class down past the
# 1e-7 clamp (ln 1e-7 = -16.1: -13 stays 17 x above it, -19 and below are clamped in every frame)
_LADDER_D = [-120., -40., -30., -8., -3., 0., 3., 8., 30., 120.]
_LADDER_S = [0., -2., -5., -10., -13., -19., -25., -40., -90., -120.]
_LADDER_D16 = _LADDER_D + [-60., -20., -1., 1., 20., 60.]
_LADDER_S16 = _LADDER_S + [-1., -7., -22., -30., -60., -100.]


def steer_heads(params, steering):
    """The four head tensors of ``params`` moved into a confident regime (a randomly initialised CRNN keeps every posterior in
    0.4 .. 0.6 and no attention value near the clamp); everything in front of the heads stays as make_params gives it.
    "ladder": exact saturation - posteriors exactly 0 and 1, attention clamped in every frame of half the classes;
    "confident": no cliff - at the shapes of tests/test_gpu_heads_regimes.py, in eval mode and in train mode without dropout,
    posteriors between 1.4e-4 and 1 - 1.8e-4 (the widest: (2, 1040), train mode) and 9 - 19 % of the attention clamped at
    (3, 136) and (2, 1040) (profiles/heads_regimes.md has the table).  Returns a new dict."""
    out = dict(params)
    if steering is None:
        return out
    nc = params["dense.bias"].numel()
    dt = params["dense.bias"].dtype
    if steering == "ladder":
        d, s = {1: ([30.], [0.]), 10: (_LADDER_D, _LADDER_S), 16: (_LADDER_D16, _LADDER_S16)}[nc]
        out["dense.weight"] = params["dense.weight"] * 0.25
        out["dense.bias"] = torch.tensor(d, dtype=dt)
        out["dense_softmax.bias"] = torch.tensor(s, dtype=dt)
    elif steering == "confident":
        out["dense.weight"] = params["dense.weight"] * 12
        out["dense.bias"] = torch.linspace(-5, 5, nc, dtype=torch.float64).to(dt)
        out["dense_softmax.weight"] = params["dense_softmax.weight"] * 30
        out["dense_softmax.bias"] = torch.linspace(6, -6, nc, dtype=torch.float64).to(dt)
    else:
        raise ValueError(steering)
    return out


def steer_model(model, params, steering):
    """steer_heads on ``params`` and the same four tensors written into ``model`` (in place); returns the steered params."""
    out = steer_heads(params, steering)
    named = dict(model.named_parameters())
    with torch.no_grad():
        for n in HEAD_NAMES:
            named[n].copy_(out[n])
    return out


def set_bn(model, bn_state):
    bufs = dict(model.named_buffers())
    with torch.no_grad():
        for k, v in bn_state.items():
            bufs[k].copy_(v.to(bufs[k].device))


def oracle_masks(seed, B, T, p, C=64, H=64):
    """The four dropout masks the HIP kernels draw for Philox key ``seed`` (oracle/philox.py)."""
    if p <= 0:
        return None
    H1, H2, T3 = T // 2, T // 4, T // 8
    return {
        "drop0": torch.tensor(philox.dropout_mask_pooled(seed, 0, B, T, 64, C, p)),
        "drop1": torch.tensor(philox.dropout_mask_pooled(seed, 1, B, H1, 16, C, p)),
        "drop2": torch.tensor(philox.dropout_mask_pooled(seed, 2, B, H2, 4, C, p)),
        "drop_rnn": torch.tensor(philox.dropout_mask_flat(seed, 8, (B, T3, 2 * H), p)),
    }


def seed_tensor(seed, device="cuda"):
    return torch.tensor([seed], dtype=torch.int64, device=device)


def nchw(t_nhwc):
    return t_nhwc.permute(0, 3, 1, 2)


def report(name, got, want):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    scale = np.abs(want).max() + 1e-30
    print(f"[parity] {name:34s} max|err| {err.max():.3e}  rel-to-max {err.max() / scale:.3e}  |want|max {scale:.3e}")
    return err.max(), err.max() / scale


def grads_dict(model):
    return {n: p.grad.detach().float().cpu() for n, p in model.named_parameters()}


def bn_state_from_model(model):
    return {k: v.detach().cpu().clone() for k, v in model.named_buffers()}

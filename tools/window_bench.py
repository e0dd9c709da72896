"""What training on windows of long recordings costs per step: one epoch through a longrec.WindowedFeatureSet (random crops
gathered from the recordings in HBM, labels sliced from the timelines by the same launch) against the only earlier route - the
same epoch's windows cut on the host and uploaded as clips of a plain resident.ResidentFeatureSet.

  pool      [3 600 weak clips | 7 200 unlabelled clips | --recordings recordings of --minutes minutes] (enough clips that the
            recordings' windows set the epoch's length), batches of B/4 + B/2 + B/4, sampling="random", default hop
  legs      both front-ends are built and warmed first, then --rounds times one full windowed epoch and one full pre-cut
            epoch are timed back to back (device events): ms / step of either (median), the ratio, and each leg's spread over
            the rounds, (max - min) / median.  The pre-cut set holds epoch 0's windows; its later epochs permute the same crops
            (that route freezes them), which is what the timing needs: the same shapes and the same arithmetic per window
  also      the two pools' bytes (features + labels), and the host time the old route pays for an epoch of FRESH crops:
            cutting every window and its labels and uploading them as a new set (a host clock around work that ends in a
            device synchronise)

Usage: python tools/window_bench.py [--shapes 24:f32,64:bf16] [--recordings 100] [--minutes 3] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench                                                    # noqa: E402  (build_models of the mt-* legs)
from dcase2019_task4_amd.features import Scaler  # noqa: E402
from dcase2019_task4_amd.longrec import WindowedFeatureSet  # noqa: E402
from dcase2019_task4_amd.resident import ResidentFeatureSet, ResidentFrontEnd  # noqa: E402
from dcase2019_task4_amd.train import MeanTeacherStep  # noqa: E402

T, N_MELS, NCLASS, POOL = 628, 64, 10, 8
T3 = T // POOL
FRAMES_PER_S = 16000 / 255                                      # the 16 kHz / hop 255 setting behind the 628-frame clip


def synthetic_items(n_rec, minutes, clips=(3600, 7200), seed=0):
    """Linear-mel clips of T frames (weak tags, unlabelled) and recordings of ``minutes`` minutes with strong timelines."""
    rs = np.random.RandomState(seed)
    L_rec = int(minutes * 60 * FRAMES_PER_S)
    lengths = [T] * sum(clips) + [L_rec] * n_rec
    flat = np.random.default_rng(seed).random(int(np.sum(lengths)) * N_MELS, dtype=np.float32)
    flat *= 3.0
    offs = np.r_[0, np.cumsum(lengths)[:-1]] * N_MELS
    feats = [flat[o:o + l * N_MELS].reshape(l, N_MELS) for o, l in zip(offs, lengths)]
    labels = [np.repeat((rs.uniform(size=(1, NCLASS)) < 0.2).astype(np.float32), T3, axis=0) for _ in range(clips[0])]
    labels += [-np.ones((T3, NCLASS), np.float32)] * clips[1]
    labels += [(rs.uniform(size=(L_rec // POOL, NCLASS)) < 0.1).astype(np.float32) for _ in range(n_rec)]
    return feats, labels, list(clips) + [n_rec]


def scaler_of(feats):
    from oracle import features_np
    sc = Scaler()
    sc.calculate_scaler([features_np.transform_chain(f[:T], T) for f in feats[:64]])
    return sc


def event_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def precut(ws, feats, labels, epoch, bs, sc):
    """The old route for one epoch of crops: every window slot's rows and label rows cut on the host, uploaded as the clips
    of a plain set (stream sizes = the windowed set's).  Returns (set, seconds)."""
    t0 = time.perf_counter()
    starts = ws.slot_starts(epoch)
    cut_f, cut_y = [], []
    for i, s3 in zip(ws.slot_item, starts):
        f, y = feats[i], labels[i]
        cut_f.append(f[s3 * POOL:s3 * POOL + T])
        rows = y[s3:s3 + T3]
        cut_y.append(rows if rows.shape[0] == T3 else np.concatenate([rows, np.zeros((T3 - rows.shape[0], NCLASS), np.float32)]))
    rs = ResidentFeatureSet.from_arrays(cut_f, cut_y, ws.window_stream_sizes, bs, frames=T, scaler=sc, augment_type="noise")
    torch.cuda.synchronize()
    return rs, time.perf_counter() - t0


def set_bytes(rs):
    lab = rs.label_pool if getattr(rs, "label_pool", None) is not None else rs.targets
    return {"features": int(rs.pool.numel()) * 4, "labels": int(lab.numel()) * 4}


def legs(ws, plain, B, dtype, rounds):
    fes = []
    for r in (ws, plain):
        student, teacher = bench.build_models("cuda", seed=0, mfma_dtype=dtype)
        st = MeanTeacherStep(student, teacher, B, T, 210 * 100 // 2, r.weak_mask, r.strong_mask, seed=1234)
        fe = ResidentFrontEnd(st, r)
        for _ in range(10):                # eager steps + capture of the two graphs + warm replays
            fe.run()
        fes.append((st, fe))
    torch.cuda.synchronize()
    n = len(ws)
    assert n == len(plain)
    win, cut = [], []
    for _ in range(rounds):
        win.append(event_ms(fes[0][1].run, n))
        cut.append(event_ms(fes[1][1].run, n))
    for st, _ in fes:
        assert np.isfinite(st.meters()["loss"])
        st.close()
    mw, mc = float(np.median(win)), float(np.median(cut))
    return {"rounds": rounds, "steps_per_epoch": n,
            "windowed_ms_per_step_rounds": [round(v, 4) for v in win], "precut_ms_per_step_rounds": [round(v, 4) for v in cut],
            "windowed_ms_per_step": round(mw, 4), "precut_ms_per_step": round(mc, 4), "windowed_over_precut": round(mw / mc, 4),
            "windowed_spread_max_minus_min_over_median": round((max(win) - min(win)) / mw, 4),
            "precut_spread_max_minus_min_over_median": round((max(cut) - min(cut)) / mc, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="24:f32,64:bf16")
    ap.add_argument("--recordings", type=int, default=100)
    ap.add_argument("--minutes", type=float, default=3.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_bench.py measures on the GPU: none found")
    t0 = time.perf_counter()
    feats, labels, sizes = synthetic_items(a.recordings, a.minutes)
    sc = scaler_of(feats)
    result = {"device": torch.cuda.get_device_properties(0).name,
              "command": f"python tools/window_bench.py --shapes {a.shapes} --recordings {a.recordings} --minutes {a.minutes:g} "
                         f"--rounds {a.rounds}",
              "items": {"clips": sizes[:2], "recordings": sizes[2], "recording_frames": int(feats[-1].shape[0]), "frames": T,
                        "sampling": "random"}, "legs": []}
    for shape in a.shapes.split(","):
        B, dtype = int(shape.split(":")[0]), shape.split(":")[1]
        bs = [B // 4, B // 2, B // 4]
        ws = WindowedFeatureSet.from_arrays(feats, labels, sizes, bs, T, [False, False, True], pooling_time_ratio=POOL,
                                            sampling="random", scaler=sc, augment_type="noise")
        np.random.seed(0)
        plain, recut_s = precut(ws, feats, labels, 0, bs, sc)
        recuts = [recut_s]
        for e in (1, 2):                                   # what every further epoch of fresh crops costs on the old route
            again, s = precut(ws, feats, labels, e, bs, sc)
            recuts.append(s)
            del again
        torch.cuda.empty_cache()
        leg = {"B": B, "mfma_dtype": dtype, "batch_sizes": bs, "hop_frames": ws.hop_frames,
               "windows_per_epoch": ws.window_stream_sizes, "windowed_pool_bytes": set_bytes(ws),
               "precut_pool_bytes": set_bytes(plain), "precut_recut_and_upload_s": [round(s, 3) for s in recuts],
               "precut_recut_and_upload_median_s": round(float(np.median(recuts)), 3)}
        leg.update(legs(ws, plain, B, dtype, a.rounds))
        leg["precut_recut_ms_per_step_if_fresh_each_epoch"] = round(1e3 * leg["precut_recut_and_upload_median_s"]
                                                                     / leg["steps_per_epoch"], 4)
        result["legs"].append(leg)
        print(json.dumps(leg), flush=True)
        del ws, plain
        torch.cuda.empty_cache()
    result["total_s"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

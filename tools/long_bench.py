"""What inference on recordings longer than one clip costs: inference.get_long_predictions (overlapping windows, blended
posteriors, ONE decode of the whole timeline) against the only route there was before it - the same recordings cut on the
host into disjoint `frames`-long clips, through ResidentFeatureSet.for_eval + get_predictions.  The cut-into-clips leg
produces a DIFFERENT event table (events are split at every cut and each piece is median-filtered with reflected edges): the
comparison is of cost, not of results.

Synthetic linear-mel recordings at the baseline geometry (frames = 628, 64 mel bands, 10 classes, pooling 8, batch 64):
  "1h"        one recording of 360 x 628 frames
  "100x3min"  100 recordings of 18 x 628 frames
Per workload, in ONE run, the legs alternate for --rounds rounds (default 5) after a warm-up round:
  clips        get_predictions on the for_eval set of the disjoint clips
  long_T3      get_long_predictions at hop3 = T3 (no overlap: the same number of forwards up to the padding of the last window)
  long_default get_long_predictions at the default hop (about half a window: about twice the windows)
each timed with a host clock around the call (it ends with the host copy of the event table, so it is synchronised); reported
are the median and the spread (max - min) / median of every leg.  The sets are built before the timed calls (build times are
reported once).  sed_stitch_decode alone: its four launches bracketed by a device-event pair on preallocated buffers, warm,
median of --decode-reps (default 30) single calls, for either hop.

The clips leg needs nothing this tool's commit added, so the tool also runs on a tree without the long path (it then reports
that leg only).

Usage: python tools/long_bench.py [--rounds 5] [--decode-reps 30] [--out profiles/long_inference.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench                                                    # noqa: E402  (build_models)
from dcase2019_task4_amd import _lib, inference  # noqa: E402
from dcase2019_task4_amd.features import Scaler  # noqa: E402
from dcase2019_task4_amd.resident import ResidentFeatureSet  # noqa: E402

T, N_MELS, NCLASS, POOL, BATCH = 628, 64, 10, 8, 64
WORKLOADS = {"1h": (1, 360), "100x3min": (100, 18)}            # recordings, clips of T frames per recording
HAVE_LONG = hasattr(inference, "get_long_predictions")


class _Clips:
    """DataLoadDf-like: what ResidentFeatureSet.for_eval reads."""

    def __init__(self, clips, names):
        self.clips, self.filenames = clips, pd.Series(names)

    def __len__(self):
        return len(self.clips)

    def get_sample(self, i):
        return self.clips[i], None


class _Enc:
    labels = [f"class_{i}" for i in range(NCLASS)]

    def decode_strong(self, m):
        raise RuntimeError("the device decode is used")


def recordings(n_rec, clips_per_rec, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.random((clips_per_rec * T, N_MELS), dtype=np.float32) * 3.0 for _ in range(n_rec)]


def scaler_of(rec):
    from oracle import features_np
    sc = Scaler()
    sc.calculate_scaler([features_np.transform_chain(rec[k * T:(k + 1) * T], T) for k in range(min(16, len(rec) // T))])
    return sc


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    med = float(np.median(v))
    return {"median_ms": med, "spread": float((v.max() - v.min()) / med), "samples_ms": [float(x) for x in v]}


def decode_alone(model, ls, reps):
    """The four launches of sed_stitch_decode on the set's real window posteriors, one device-event pair per call."""
    _, _, win_strong = inference.get_long_predictions(model, ls, _Enc.labels, batch_size=BATCH, return_posteriors=True)
    l, dev, ptr = _lib.lib(), win_strong.device, _lib.ptr
    total, n_rec, cap = ls.total_frames, ls.n_rec, ls.capacity(NCLASS)
    thr = torch.full((NCLASS,), 0.5, device=dev)
    win = torch.full((NCLASS,), 5, dtype=torch.int32, device=dev)
    timeline = torch.empty(total, NCLASS, device=dev)
    ev_ptr = torch.empty(n_rec * NCLASS + 1, dtype=torch.int64, device=dev)
    ev_pairs = torch.empty(cap, 2, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(l.sed_stitch_decode_ws_bytes(total, n_rec, NCLASS), dtype=torch.uint8, device=dev)

    def call():
        _lib.check(l.sed_stitch_decode(ptr(win_strong), ptr(ls.rec_win0), ptr(ls.rec_frame0), n_rec, ls.T3, NCLASS, ls.hop3, 1,
                                       ptr(thr), ptr(win), ptr(timeline), None, ptr(ev_ptr), ptr(ev_pairs), cap, ptr(ws),
                                       ws.numel(), ptr(err), _lib.stream_ptr()), "sed_stitch_decode")
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    assert int(err.item()) == 0
    s = stats(ms)
    return {"median_ms": s["median_ms"], "spread": s["spread"], "reps": reps, "timeline_frames": total, "windows": ls.n_clips,
            "events": int(ev_ptr[-1].item())}


def workload(name, model, rounds, reps):
    n_rec, per = WORKLOADS[name]
    recs = recordings(n_rec, per)
    sc = scaler_of(recs[0])
    names = [f"{name}_{r}.wav" for r in range(n_rec)]
    out = {"recordings": n_rec, "feature_frames_each": per * T, "seconds_each": per * T * 255 / 16000.0}
    t0 = time.perf_counter()
    clips = _Clips([rec[k * T:(k + 1) * T] for rec in recs for k in range(per)],
                   [f"{n}#{k}" for n in names for k in range(per)])
    cs = ResidentFeatureSet.for_eval(clips, T, scaler=sc)
    torch.cuda.synchronize()
    out["clips_set_build_ms"] = (time.perf_counter() - t0) * 1e3
    enc = _Enc().decode_strong
    legs = {"clips": lambda: inference.get_predictions(model, cs, enc, POOL, batch_size=BATCH)}
    rows = {}
    if HAVE_LONG:
        sets = {}
        for leg, hop in (("long_T3", (T // POOL) * POOL), ("long_default", None)):
            t0 = time.perf_counter()
            sets[leg] = inference.LongRecordingSet.from_arrays(recs, T, hop_frames=hop, scaler=sc, filenames=names)
            torch.cuda.synchronize()
            out[leg + "_set_build_ms"] = (time.perf_counter() - t0) * 1e3
            out[leg + "_windows"] = sets[leg].n_clips
            legs[leg] = (lambda s: lambda: inference.get_long_predictions(model, s, enc, POOL, batch_size=BATCH))(sets[leg])
    out["clips_forwarded"] = len(clips)
    for leg, fn in legs.items():                                 # warm-up round: every shape, every code object
        rows[leg] = len(fn())
    ms = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg, fn in legs.items():
            ms[leg].append(wall_ms(fn))
    for leg in legs:
        out[leg] = dict(stats(ms[leg]), event_rows=rows[leg])
    if HAVE_LONG:
        for leg in ("long_T3", "long_default"):
            out[leg]["ratio_to_clips"] = out[leg]["median_ms"] / out["clips"]["median_ms"]
            out[leg]["stitch_decode_alone"] = decode_alone(model, sets[leg], reps)
        out["long_default"]["window_ratio_to_long_T3"] = out["long_default_windows"] / out["long_T3_windows"]
        out["long_default"]["ratio_to_long_T3"] = out["long_default"]["median_ms"] / out["long_T3"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--decode-reps", type=int, default=30)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "long_inference.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("long_bench.py measures on the GPU: no device found (nothing is measured on a CPU)")
    if args.rounds < 5 or args.decode_reps < 20:
        raise SystemExit("need --rounds >= 5 and --decode-reps >= 20")
    model, _ = bench.build_models("cuda", seed=0, mfma_dtype="f32")
    model.eval()
    result = {"tool": "tools/long_bench.py", "device": torch.cuda.get_device_name(0), "frames": T, "batch_size": BATCH,
              "model": "baseline CRNN, fp32 kernel set, eval mode", "rounds": args.rounds, "long_path_present": HAVE_LONG,
              "timing": "host clock around each synchronised call, legs alternated; decode alone: device events",
              "note": "the clips leg yields a different event table (events split at the cuts); rows are reported, not compared",
              "not_measured": ["from_waveforms / feature extraction", "other batch sizes, bf16 / wide models",
                               "recordings longer than 1 h", "a run with the GPU to itself (the host is shared)"],
              "workloads": {}}
    for name in args.workloads.split(","):
        result["workloads"][name] = workload(name, model, args.rounds, args.decode_reps)
        print(json.dumps({name: result["workloads"][name]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

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

  --events  the legs of sampling="events" instead, on the same pool with sparse strong timelines (their density is in the
            result): (a) slot_starts on the device against the label pool copied back and the definition restated with numpy
            cumulative sums, identical starts asserted; (b) the two entries alone; (c) ms / step of an epoch with "events"
            against "random"; (d) the share of windows that hold an active label frame, exactly, from the tables.  Legs
            alternate in one run, --rounds rounds, medians, spread = (max - min) / median

Usage: python tools/window_bench.py [--events] [--shapes 24:f32,64:bf16] [--recordings 100] [--minutes 3] [--rounds 5]
                                    [--out FILE]"""
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


# ---- --events: event-aware crop sampling ---------------------------------------------------------------------------------------
def sparse_timelines(n_rec, rows, seed=1):
    """Strong timelines with few events: per recording 2 - 4 events, each of one random class and 4 - 40 label frames."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n_rec):
        y = np.zeros((rows, NCLASS), np.float32)
        for _ in range(rs.randint(2, 5)):
            n = int(rs.randint(4, 41))
            on = int(rs.randint(0, rows - n))
            y[on:on + n, rs.randint(NCLASS)] = 1
        out.append(y)
    return out


def host_event_starts(ws, epoch):
    """The only other route to the starts of sampling="events": the label pool copied to the host, the definition restated
    with numpy cumulative sums per item, the same draws."""
    pool = ws.label_pool.cpu().numpy()
    u, v, m = ws.event_draws(epoch)
    start = np.zeros(len(ws.slot_item), dtype=np.int64)
    first = np.r_[0, np.cumsum(ws.n_w_host)]
    for i in np.flatnonzero(ws.item_windowed):
        lo, R, hi = int(ws.label_offset_host[i]), int(ws.label_rows_host[i]), int(ws.start_hi_host[i])
        A = np.concatenate([np.zeros((1, ws.nclass), np.int64), np.cumsum(pool[lo:lo + R] > 0, axis=0)])
        s = np.arange(hi + 1)
        C = np.cumsum(A[np.minimum(s + ws.T3, R)] - A[np.minimum(s, R)], axis=0)
        present = np.flatnonzero(C[hi] > 0)
        for j in range(first[i], first[i + 1]):
            if not m[j] or present.size == 0:
                start[j] = (int(u[j]) * (hi + 1)) >> 64
            else:
                c = present[int(v[j]) % present.size]
                start[j] = np.searchsorted(C[:, c], (int(u[j]) * int(C[hi, c])) >> 64, side="right")
    return start


def spread(vals):
    return round((max(vals) - min(vals)) / float(np.median(vals)), 4)


def covered_share(ws, labels, epochs):
    """The share of the windowed streams' windows that hold at least one active label frame, exactly, over ``epochs``."""
    hit = n = 0
    slots = np.flatnonzero(ws.item_windowed[ws.slot_item])
    for e in epochs:
        starts = ws.slot_starts(e)
        for j in slots:
            hit += bool((labels[ws.slot_item[j]][starts[j]:starts[j] + T3] > 0).any())
        n += len(slots)
    return round(hit / n, 4)


def step_legs(sets, B, dtype, rounds):
    """ms / step of one epoch through each set's front-end, the legs alternated in every round."""
    fes = []
    for r in sets:
        student, teacher = bench.build_models("cuda", seed=0, mfma_dtype=dtype)
        st = MeanTeacherStep(student, teacher, B, T, 210 * 100 // 2, r.weak_mask, r.strong_mask, seed=1234)
        fe = ResidentFrontEnd(st, r)
        for _ in range(10):
            fe.run()
        fes.append((st, fe))
    torch.cuda.synchronize()
    n = len(sets[0])
    times = [[] for _ in sets]
    for _ in range(rounds):
        for k, (_, fe) in enumerate(fes):
            times[k].append(event_ms(fe.run, n))
    for st, _ in fes:
        assert np.isfinite(st.meters()["loss"])
        st.close()
    return n, times


def events_main(a):
    t0 = time.perf_counter()
    feats, labels, sizes = synthetic_items(a.recordings, a.minutes)
    n_clip = sizes[0] + sizes[1]
    labels = labels[:n_clip] + sparse_timelines(a.recordings, labels[-1].shape[0])
    sc = scaler_of(feats)
    rec = np.stack(labels[n_clip:])
    result = {"device": torch.cuda.get_device_properties(0).name,
              "command": f"python tools/window_bench.py --events --shapes {a.shapes} --recordings {a.recordings} "
                         f"--minutes {a.minutes:g} --rounds {a.rounds}",
              "items": {"clips": sizes[:2], "recordings": sizes[2], "recording_frames": int(feats[-1].shape[0]), "frames": T,
                        "label_rows_per_recording": int(rec.shape[1]),
                        "labels": "2 - 4 events per recording, one random class each, 4 - 40 label frames long",
                        "active_share_of_label_cells": round(float((rec > 0).mean()), 6),
                        "share_of_label_rows_with_an_active_class": round(float((rec > 0).any(axis=2).mean()), 4)},
              "legs": []}

    def build(sampling, bs, fraction=0.5):
        return WindowedFeatureSet.from_arrays(feats, labels, sizes, bs, T, [False, False, True], pooling_time_ratio=POOL,
                                              sampling=sampling, scaler=sc, augment_type="noise", event_fraction=fraction)

    first = True
    for shape in a.shapes.split(","):
        B, dtype = int(shape.split(":")[0]), shape.split(":")[1]
        bs = [B // 4, B // 2, B // 4]
        ev, rnd = build("events", bs), build("random", bs)
        leg = {"B": B, "mfma_dtype": dtype, "batch_sizes": bs, "window_slots": int(len(ev.slot_item)),
               "windowed_slots": int(ev.item_windowed[ev.slot_item].sum()), "event_fraction": ev.event_fraction}
        if first:                                       # (a), (b), (d) do not depend on the batch shape: measured once
            first = False
            ev.slot_starts(0)
            host_event_starts(ev, 0)                    # both routes warm
            dev_s, host_s = [], []
            for r in range(a.rounds):
                t = time.perf_counter()
                got = ev.slot_starts(r)
                dev_s.append(time.perf_counter() - t)
                t = time.perf_counter()
                want = host_event_starts(ev, r)
                host_s.append(time.perf_counter() - t)
                assert np.array_equal(got, want), "the device starts differ from the host restatement"
            leg["a_slot_starts_ms"] = {"device_rounds": [round(1e3 * s, 3) for s in dev_s],
                                       "host_rounds": [round(1e3 * s, 3) for s in host_s],
                                       "device": round(1e3 * float(np.median(dev_s)), 3),
                                       "host": round(1e3 * float(np.median(host_s)), 3),
                                       "device_spread": spread(dev_s), "host_spread": spread(host_s),
                                       "identical_starts": True, "clock": "host, around a call that ends with the starts on the host"}
            tab = ev._crop_tables()
            draws = ev._event_upload(0)
            for _ in range(3):
                ev._event_launch(tab, *draws)
            alone = [event_ms(lambda: ev._event_launch(tab, *draws), 1) for _ in range(30)]
            leg["b_two_entries_ms"] = {"median_of_30": round(float(np.median(alone)), 4), "min": round(min(alone), 4),
                                       "max": round(max(alone), 4), "launches": 6, "clock": "device events around one call of each"}
            epochs = range(5)
            share = {"random": covered_share(rnd, labels, epochs)}
            for f in (0.5, 1.0):
                ev.event_fraction = f
                share[f"events_{f:g}"] = covered_share(ev, labels, epochs)
            ev.event_fraction = 0.5
            leg["d_share_of_windows_with_an_active_frame"] = dict(share, epochs=len(epochs), exact=True)
        n, (t_ev, t_rnd) = step_legs([ev, rnd], B, dtype, a.rounds)
        m_ev, m_rnd = float(np.median(t_ev)), float(np.median(t_rnd))
        band = max(max(t_ev) - min(t_ev), max(t_rnd) - min(t_rnd))
        leg["c_ms_per_step"] = {"steps_per_epoch": n, "events_rounds": [round(v, 4) for v in t_ev],
                                "random_rounds": [round(v, 4) for v in t_rnd], "events": round(m_ev, 4), "random": round(m_rnd, 4),
                                "events_spread": spread(t_ev), "random_spread": spread(t_rnd),
                                "difference": round(m_ev - m_rnd, 4), "larger_max_minus_min": round(band, 4),
                                "difference_outside_the_band": bool(abs(m_ev - m_rnd) > band)}
        result["legs"].append(leg)
        print(json.dumps(leg), flush=True)
        del ev, rnd
        torch.cuda.empty_cache()
    result["not_measured"] = "other nclass, the 1 h recording, the kernels one by one"
    result["total_s"] = round(time.perf_counter() - t0, 1)
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="24:f32,64:bf16")
    ap.add_argument("--recordings", type=int, default=100)
    ap.add_argument("--minutes", type=float, default=3.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--events", action="store_true", help='the legs of sampling="events" instead (profiles/window_events.json)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_bench.py measures on the GPU: none found")
    if a.events:
        return events_main(a)
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

"""CPU checks of longrec.WindowedFeatureSet: its epoch tables against ResidentFeatureSet's (non-windowed streams) and against
the plain-loop statement of tests/window_np.py (window counts, grid and random starts), rank shares, encode_timeline against
a restated ManyHotEncoder.encode_strong_df, and input validation.  (A set on a CPU device builds everything but refuses to
gather.)"""
import numpy as np
import pandas as pd
import pytest

from dcase2019_task4_amd import _lib
from dcase2019_task4_amd import dist as sdist
from dcase2019_task4_amd.features import FeatureConfig
from dcase2019_task4_amd.inference import WindowedFeatureSet as exported_with_long_recording_set
from dcase2019_task4_amd.longrec import WindowedFeatureSet, encode_timeline, window_plan
from dcase2019_task4_amd.resident import ResidentFeatureSet
from tests import window_np as wn

FRAMES, POOL, T3 = 32, 4, 8
LENGTHS = [1, 31, 32, 33, 100, 259]


def _items(lengths, seed=0, n_mels=4, nclass=3, pool=POOL):
    rs = np.random.RandomState(seed)
    feats = [np.abs(rs.standard_normal((n, n_mels))).astype(np.float32) for n in lengths]
    labels = [rs.uniform(size=(max(1, n // pool), nclass)).astype(np.float32) for n in lengths]
    return feats, labels


def _clip_arrays(sizes, seed=0):
    """The ragged clips of tests/test_resident_cpu.py::_arrays, with a one-row timeline per clip."""
    rs = np.random.RandomState(seed)
    n = sum(sizes)
    feats = [np.abs(rs.standard_normal((int(rs.randint(3, 9)), 4))).astype(np.float32) for _ in range(n)]
    tgts = [rs.uniform(size=(2, 3)).astype(np.float32) for _ in range(n)]
    return feats, tgts


def test_exported_beside_long_recording_set():
    assert exported_with_long_recording_set is WindowedFeatureSet and issubclass(WindowedFeatureSet, ResidentFeatureSet)


@pytest.mark.parametrize("sizes,batch_sizes", [((31, 50, 27), (6, 12, 6)), ((29, 77), (6, 18))])
def test_non_windowed_streams_follow_the_resident_set(sizes, batch_sizes):
    """windowed = [False, ...]: under the same np.random.seed the item column is ResidentFeatureSet.epoch_rows, start3 is 0."""
    feats, tgts = _clip_arrays(sizes)
    plain = ResidentFeatureSet.from_arrays(feats, tgts, sizes, batch_sizes, frames=6, device="cpu")
    for sampling in ("random", "grid"):
        ws = WindowedFeatureSet.from_arrays(feats, tgts, sizes, batch_sizes, 6, [False] * len(sizes), pooling_time_ratio=3,
                                            sampling=sampling, device="cpu")
        assert len(ws) == len(plain) and ws.batch == plain.batch and ws.target_shape == (2, 3)
        assert ws.weak_mask == plain.weak_mask and ws.strong_mask == plain.strong_mask
        np.random.seed(1234)
        want = [plain.epoch_rows() for _ in range(3)]
        np.random.seed(1234)
        got = [ws.epoch_windows(e) for e in range(3)]
        for w, g in zip(want, got):
            assert g.shape == (len(plain), sum(batch_sizes), 2)
            np.testing.assert_array_equal(g[..., 0], w)
            assert (g[..., 1] == 0).all()
        np.random.seed(1234)
        t = ws.epoch_table(0)
        assert t.dtype == np.int32 and t.flags["C_CONTIGUOUS"]
        np.testing.assert_array_equal(t, got[0])


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("sizes,batch_sizes", [((31, 50, 27), (8, 16, 8)), ((29, 77), (8, 24))])
def test_rank_shares_are_dist_shard_indices(sizes, batch_sizes, world):
    feats, tgts = _clip_arrays(sizes, 1)
    ws = WindowedFeatureSet.from_arrays(feats, tgts, sizes, batch_sizes, 6, [False] * (len(sizes) - 1) + [True],
                                        pooling_time_ratio=3, device="cpu")
    np.random.seed(7)
    rows = ws.epoch_windows(0)
    for rank in range(world):
        got = ws.local_rows(rows, rank, world)
        for col in range(2):
            want = np.array([sdist.shard_indices(list(r), list(batch_sizes), rank, world) for r in rows[..., col]])
            np.testing.assert_array_equal(got[..., col], want)
        assert got.shape == (len(ws), sum(batch_sizes) // world, 2)


def _start_rule_set(sampling, seed=3, hop_frames=None):
    feats, labels = _items(LENGTHS * 2, 5)
    return WindowedFeatureSet.from_arrays(feats, labels, [6, 6], [2, 3], FRAMES, [False, True], pooling_time_ratio=POOL,
                                          hop_frames=hop_frames, sampling=sampling, seed=seed, device="cpu")


@pytest.mark.parametrize("hop_frames", [None, 8, 32])
def test_window_counts_stream_sizes_and_grid_starts(hop_frames):
    ws = _start_rule_set("grid", hop_frames=hop_frames)
    hop3 = ws.hop3
    assert hop3 == {None: 4, 8: 2, 32: 8}[hop_frames]
    n_w = [window_plan(L, FRAMES, POOL, hop3)["n_w"] for L in LENGTHS]
    assert n_w == [wn.n_windows(L, FRAMES, POOL, hop3) for L in LENGTHS]
    np.testing.assert_array_equal(ws.n_w_host, [1] * 6 + n_w)
    assert ws.window_stream_sizes == [6, sum(n_w)] and ws.stream_sizes == [6, 6]
    assert len(ws) == ws.n_steps == min(6 // 2, sum(n_w) // 3)
    np.testing.assert_array_equal(ws.start_hi_host, [max(0, max(1, L // POOL) - T3) for L in LENGTHS] * 2)
    # every slot's start, in item order
    want = wn.item_starts(LENGTHS * 2, [False] * 6 + [True] * 6, FRAMES, POOL, hop3, "grid", 3, 0)
    for e in (0, 5):
        starts = ws.slot_starts(e)
        np.testing.assert_array_equal(starts, np.concatenate(want))
    for i, L in enumerate(LENGTHS):
        hi = wn.start_hi(L, FRAMES, POOL)
        assert want[6 + i] == [min(j * hop3, hi) for j in range(n_w[i])]
        assert want[6 + i][-1] == hi                       # the grid reaches the item's last label frame
    # the tables hold exactly these (item, start) pairs
    np.random.seed(11)
    t = ws.epoch_windows(0)
    legal = {(i, s) for i, ss in enumerate(want) for s in ss}
    assert {tuple(r) for r in t.reshape(-1, 2)} <= legal
    assert (t[:, :2, 0] < 6).all() and (t[:, 2:, 0] >= 6).all()


def test_random_starts_follow_the_seeded_generator_and_leave_the_global_draws_alone():
    rnd, grid = _start_rule_set("random"), _start_rule_set("grid")
    np.random.seed(99)
    tr = [rnd.epoch_windows(e) for e in range(2)]
    after_random = np.random.uniform()
    np.random.seed(99)
    tg = [grid.epoch_windows(e) for e in range(2)]
    after_grid = np.random.uniform()
    assert after_random == after_grid                      # the same number of global draws
    for a, b in zip(tr, tg):
        np.testing.assert_array_equal(a[..., 0], b[..., 0])
    # starts: the plain-loop statement's, per (seed, epoch); legal; different between epochs; reproducible
    for e in range(3):
        want = np.concatenate(wn.item_starts(LENGTHS * 2, [False] * 6 + [True] * 6, FRAMES, POOL, rnd.hop3, "random", 3, e))
        np.testing.assert_array_equal(rnd.slot_starts(e), want)
        hi = rnd.start_hi_host[rnd.slot_item]
        assert (want >= 0).all() and (want <= hi).all() and (want[:6] == 0).all()
    assert not np.array_equal(rnd.slot_starts(0), rnd.slot_starts(1))
    np.testing.assert_array_equal(rnd.slot_starts(1), rnd.slot_starts(1))
    assert not np.array_equal(rnd.slot_starts(0), _start_rule_set("random", seed=4).slot_starts(0))
    np.random.seed(99)
    np.testing.assert_array_equal(_start_rule_set("random").epoch_windows(0), tr[0])
    # an item with L3 >= T3 never yields a window with padded label frames
    L3 = np.maximum(1, np.array(LENGTHS * 2) // POOL)
    for e in range(4):
        s = rnd.slot_starts(e)
        full = L3[rnd.slot_item] >= T3
        assert (s[full] + T3 <= L3[rnd.slot_item][full]).all()


def test_every_rank_draws_the_same_global_table_and_checks_its_share():
    """Two sets built alike (as two ranks build them) draw the same global table: it depends on (global seed, set seed, epoch)
    alone, and ranks differ only in the columns they take (test_rank_shares_are_dist_shard_indices)."""
    a, b = _start_rule_set("random"), _start_rule_set("random")
    np.random.seed(5)
    ga = a.epoch_windows(1)
    np.random.seed(5)
    gb = b.epoch_windows(1)
    np.testing.assert_array_equal(ga, gb)
    np.random.seed(5)
    t = a.epoch_table(1)
    np.testing.assert_array_equal(t, ga)
    # the table check: every row is a real frame of its item
    L = a.clip_frames_host[t[..., 0]]
    assert (t[..., 0] >= 0).all() and (t[..., 0] < a.n_clips).all() and (t[..., 1] >= 0).all() and (t[..., 1] * POOL < L).all()
    for bad in ([[12, 0]], [[-1, 0]], [[0, 1]], [[5, 65]], [[5, -1]]):
        with pytest.raises(_lib.SedError):
            a.check_windows(bad)
    a.check_windows([[5, 64], [0, 0], [1, 7]])


class _Encoder:
    """ManyHotEncoder.encode_strong_df (utils/utils.py:86-94) on a DataFrame of one file's events, already in frames."""

    def __init__(self, labels, n_frames):
        self.labels, self.n_frames = list(labels), n_frames

    def encode_strong_df(self, label_df):
        y = np.zeros((self.n_frames, len(self.labels)))
        for _, row in label_df.iterrows():
            if not pd.isna(row["event_label"]):
                i = self.labels.index(row["event_label"])
                onset = int(row["onset"])
                offset = int(row["offset"])
                y[onset:offset, i] = 1
        return y


@pytest.mark.parametrize("cfg", [FeatureConfig.baseline_16k(), FeatureConfig()], ids=["16k_hop255", "44k_hop511"])
def test_encode_timeline_restates_the_reference(cfg):
    labels, pool = ["a", "b", "c"], 8
    L = 3000
    L3 = max(1, L // pool)
    sec = pool * cfg.hop_length / cfg.sample_rate                     # one label frame
    boundary = [k * pool * cfg.hop_length / cfg.sample_rate for k in (1, 7, 100, 251)]
    df = pd.DataFrame({
        "filename": ["f"] * 9,
        "onset": [0.0, 1.3, boundary[0], boundary[2], (L3 - 2.5) * sec, 2.5, 4.0, np.nan, (L3 + 5) * sec],
        "offset": [0.7, 1.3, boundary[1], boundary[3], (L3 + 40) * sec, 2.5 + sec / 3, 9.0, np.nan, (L3 + 9) * sec],
        "event_label": ["a", "b", "c", "a", "b", "c", np.nan, np.nan, "a"]})
    got = encode_timeline(df, L3, labels, cfg, pool)
    frames_df = df.copy()
    frames_df.onset = frames_df.onset * cfg.sample_rate // cfg.hop_length // pool          # main.py:227-228
    frames_df.offset = frames_df.offset * cfg.sample_rate // cfg.hop_length // pool
    want = _Encoder(labels, L3).encode_strong_df(frames_df)
    assert got.dtype == np.float32 and got.shape == (L3, 3)
    np.testing.assert_array_equal(got, want)
    assert got[:, 1].sum() == 3 and got[-3:, 1].all()                 # straddling the end: the rows that exist
    # tuples instead of a DataFrame, and a file without events
    tup = [(r.onset, r.offset, r.event_label) for r in df.itertuples()]
    np.testing.assert_array_equal(encode_timeline(tup, L3, labels, cfg, pool), want)
    assert not encode_timeline(df.iloc[:0], 5, labels, cfg, pool).any()


def test_from_events_builds_one_timeline_per_item():
    cfg, labels, pool = FeatureConfig.baseline_16k(), ["a", "b"], 4
    feats, _ = _items([100, 40, 7, 64], 2)
    names = ["r0", "r1", "r2", "r3"]
    sec = pool * cfg.hop_length / cfg.sample_rate
    ev = pd.DataFrame({"filename": ["r0", "r0", "r3", "r1"], "onset": [2.2 * sec, 10.5 * sec, 0.0, np.nan],
                       "offset": [6.1 * sec, 400 * sec, 3.5 * sec, np.nan], "event_label": ["a", "b", "b", np.nan]})
    ws = WindowedFeatureSet.from_events(feats, ev, names, labels, cfg, [4], [2], 32, [True], pooling_time_ratio=pool,
                                        device="cpu")
    np.testing.assert_array_equal(ws.label_rows_host, [25, 10, 1, 16])
    np.testing.assert_array_equal(ws.label_offset_host, [0, 25, 35, 36])
    pool_np = ws.label_pool.numpy()
    assert pool_np.shape == (52, 2) and ws.filenames == names
    for i, name in enumerate(names):
        want = encode_timeline(ev[ev.filename == name], ws.label_rows_host[i], labels, cfg, pool)
        o = ws.label_offset_host[i]
        np.testing.assert_array_equal(pool_np[o:o + ws.label_rows_host[i]], want)
    assert pool_np[2:6, 0].all() and pool_np[10:25, 1].all() and not pool_np[25:36].any() and pool_np[36:39, 1].all()


def test_bad_inputs_raise():
    feats, labels = _items(LENGTHS, 1)
    ok = dict(stream_sizes=[3, 3], batch_sizes=[1, 1], frames=FRAMES, windowed=[False, True], pooling_time_ratio=POOL,
              device="cpu")
    WindowedFeatureSet.from_arrays(feats, labels, **ok)
    with pytest.raises(ValueError, match="label timelines"):
        WindowedFeatureSet.from_arrays(feats, labels[:-1], **ok)
    bad = list(labels)
    bad[2] = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="labels of shape"):
        WindowedFeatureSet.from_arrays(feats, bad, **ok)
    with pytest.raises(ValueError, match="windowed"):
        WindowedFeatureSet.from_arrays(feats, labels, **dict(ok, windowed=[True]))
    with pytest.raises(ValueError, match="sampling"):
        WindowedFeatureSet.from_arrays(feats, labels, sampling="dense", **ok)
    with pytest.raises(ValueError, match="hop_frames"):
        WindowedFeatureSet.from_arrays(feats, labels, hop_frames=6, **ok)
    with pytest.raises(ValueError, match="batch sizes"):
        WindowedFeatureSet.from_arrays(feats, labels, **dict(ok, batch_sizes=None))
    with pytest.raises(ValueError):                                        # a stream with fewer windows than its batch size
        WindowedFeatureSet.from_arrays(feats, labels, **dict(ok, batch_sizes=[4, 1]))
    with pytest.raises(TypeError):
        WindowedFeatureSet.from_arrays(feats, labels, augment="mixup", **ok)


def test_the_clip_interface_refuses_a_windowed_set():
    """The base class's clip-index gather, eval_batch and epoch_rows must not address items as clips - also on a CPU set,
    where nothing gathers at all."""
    import torch
    feats, labels = _items(LENGTHS, 1)
    ws = WindowedFeatureSet.from_arrays(feats, labels, [3, 3], [1, 1], FRAMES, [False, True], pooling_time_ratio=POOL,
                                        device="cpu")
    out = torch.empty(2, 1, FRAMES, 4)
    with pytest.raises(_lib.SedError):
        ws.gather(torch.zeros(2, dtype=torch.int32), out)
    with pytest.raises(_lib.SedError):
        ws.eval_batch(0, 2)
    with pytest.raises(ValueError):
        ws.epoch_rows()
    with pytest.raises(_lib.SedError):
        ws.transform([[0, 0]], seed=1)                                     # a CPU set refuses to gather


def test_entry_point_refuses_null_arguments_without_a_gpu():
    l = _lib.lib()
    assert l.sed_gather_window_logmel_transform(None, None, None, 1, 8, None, 2, 64, 628, 8, None, None, None, None, None, None,
                                                None, None, 78, 10, None, None, 0, 0, None) != 0
    assert b"sed_gather_window_logmel_transform" in l.sed_last_error()

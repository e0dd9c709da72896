"""The plain-loop statement of sed_events_rasterize (tests/rasterize_np.py) checked on its own - against encode_timeline on
hand cases, the idempotence of replace, the maximum of two tables against the rasterised union, the hand cases of the error
bits - and what needs no GPU of the fronts: the host refusals of ``relabel`` on a CPU-device set, the argument checks of the
C entry that return before any launch, ``rows_overlap``."""
import numpy as np
import pytest
import torch

from tests import rasterize_np as rn


class _Cfg:
    sample_rate = 44100
    hop_length = 511


LABELS = ["a", "b", "c"]
SEC = 511 * 8 / 44100                                                          # one label frame at pooling ratio 8


def _seconds(frame):
    """A time that lies safely inside label frame ``frame`` (encode_timeline floors twice)."""
    return (frame + 0.25) * SEC


def test_the_statement_equals_encode_timeline_on_hand_cases():
    from dcase2019_task4_amd.longrec import encode_timeline
    L3 = 40
    cols = [[(0, 3), (3, 9), (20, 21)], [], [(5, 40)]]                         # row 0, touching, one row; empty; up to L3
    events = [(_seconds(on), _seconds(off), LABELS[c]) for c, col in enumerate(cols) for on, off in col]
    want = encode_timeline(events, L3, LABELS, _Cfg, 8)
    ptr, pairs = rn.table(cols)
    got, err, unspec = rn.rasterize(ptr, pairs, [0, L3], 1, 3, np.full((L3, 3), np.nan, np.float32))
    assert err == 0 and not unspec.any()
    rn.same_bits(got, want)
    assert want[:, 0].sum() == 10 and want[:, 1].sum() == 0 and want[:, 2].sum() == 35
    # two recordings, placed by dst_row0 in the other order with a gap that keeps its bytes
    cols2 = cols + [[(1, 2)], [(0, 7)], []]
    ptr, pairs = rn.table(cols2)
    dst = np.full((60, 3), -7.0, np.float32)
    got, err, _ = rn.rasterize(ptr, pairs, [0, L3, L3 + 7], 2, 3, dst, dst_row0=[15, 2])
    assert err == 0
    rn.same_bits(got[15:55], want)
    rn.same_bits(got[2:9], encode_timeline([(_seconds(1), _seconds(2), "a"), (_seconds(0), _seconds(7), "b")], 7, LABELS, _Cfg, 8))
    assert (got[:2] == -7).all() and (got[9:15] == -7).all() and (got[55:] == -7).all()


def test_replace_is_idempotent_and_values_and_points_are_carried():
    cols = [[(0, 2), (4, 5)], [(1, 3)], [(0, 6)], []]                          # K = 2 points, one recording, two classes
    ptr, pairs = rn.table(cols)
    value = np.array([0.5, np.nan, -0.0, 0.25], np.float32)
    value[1] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    dst = np.full((6, 2), np.nan, np.float32)
    once, err, _ = rn.rasterize(ptr, pairs, [0, 6], 1, 2, dst, value=value, point=[0, 1], n_points=2)
    twice, err2, _ = rn.rasterize(ptr, pairs, [0, 6], 1, 2, once, value=value, point=[0, 1], n_points=2)
    assert err == 0 and err2 == 0
    rn.same_bits(once, twice)
    bits = once.view(np.uint32)
    assert bits[:, 0].tolist() == [0x3F000000, 0x3F000000, 0, 0, 0x7FC12345, 0]         # class 0 from point 0
    assert bits[:, 1].tolist() == [0] * 6                                      # class 1 from point 1: its column is empty
    other, _, _ = rn.rasterize(ptr, pairs, [0, 6], 1, 2, dst, value=value, point=[1, 0], n_points=2)
    assert other.view(np.uint32)[:, 0].tolist() == [0x3E800000] * 6 and other.view(np.uint32)[:, 1].tolist() == [0, 0x80000000,
                                                                                                              0x80000000, 0, 0, 0]


def test_the_maximum_of_two_tables_is_the_rasterised_union_and_keeps_what_is_larger():
    a = [[(0, 4), (10, 12)], [(3, 5)]]
    b = [[(2, 6)], [(8, 9)]]
    union = [[(0, 6), (10, 12)], [(3, 5), (8, 9)]]
    zero = np.zeros((12, 2), np.float32)
    first, e1, _ = rn.rasterize(*rn.table(a), [0, 12], 1, 2, zero)
    both, e2, _ = rn.rasterize(*rn.table(b), [0, 12], 1, 2, first, combine=rn.MAXIMUM)
    want, e3, _ = rn.rasterize(*rn.table(union), [0, 12], 1, 2, np.full((12, 2), np.nan, np.float32))
    assert e1 == e2 == e3 == 0
    rn.same_bits(both, want)
    # old contents: larger, smaller, equal, NaN and -1 under an event of value 0.5; uncovered elements stay
    old = np.array([[2.0], [0.25], [0.5], [np.nan], [-1.0], [7.0]], np.float32)
    got, err, _ = rn.rasterize(*rn.table([[(0, 5)]]), [0, 6], 1, 1, old, value=np.array([0.5], np.float32), combine=rn.MAXIMUM)
    assert err == 0 and got[[0, 1, 2, 4, 5], 0].tolist() == [2.0, 0.5, 0.5, 0.5, 7.0] and np.isnan(got[3, 0])
    nanv, _, _ = rn.rasterize(*rn.table([[(0, 5)]]), [0, 6], 1, 1, old, value=np.array([np.nan], np.float32), combine=rn.MAXIMUM)
    rn.same_bits(nanv, old)                                                    # a NaN value never replaces anything


@pytest.mark.parametrize("event,bit", [((7, 7), 64), ((9, 3), 64), ((-1, 4), 64), ((19, 21), 64), ((4, 8), 64), ((5, 8), 0)])
def test_the_error_bits_of_events_by_hand(event, bit):
    cols = [[(0, 5), event, (12, 14)], [(1, 2)]]                               # L3 = 20; (4, 8) overlaps, (5, 8) touches
    ptr, pairs = rn.table(cols)
    dst = np.full((20, 2), -7.0, np.float32)
    got, err, unspec = rn.rasterize(ptr, pairs, [0, 20], 1, 2, dst)
    assert err == bit
    assert unspec[:, 0].all() == bool(bit) and not unspec[:, 1].any()
    assert got[:, 1].tolist() == [0.0, 1.0] + [0.0] * 18                       # the other column is right either way


def test_the_error_bits_of_tables_by_hand():
    cols = [[(0, 5)], [(1, 2)], [(0, 3)], [(2, 4)]]                            # two recordings of 10 and 6 rows, two classes
    ptr, pairs = rn.table(cols)
    dst = np.full((20, 2), -7.0, np.float32)
    ok, err, _ = rn.rasterize(ptr, pairs, [0, 10, 16], 2, 2, dst)
    assert err == 0 and (ok[16:] == -7).all()
    for bad_ptr in ([0, 1, 2, 9, 4], [-1, 1, 2, 3, 4], [0, 1, 3, 2, 4]):      # beyond the capacity, negative, decreasing
        got, err, _ = rn.rasterize(np.array(bad_ptr), pairs, [0, 10, 16], 2, 2, dst)
        assert err & 16 and not err & ~(16 | 64)                               # (a shifted column may hold unsorted events)
        rn.same_bits(got[:10, 1] if bad_ptr[0] < 0 else got[:10, 0], ok[:10, 1] if bad_ptr[0] < 0 else ok[:10, 0])
    got, err, _ = rn.rasterize(ptr, pairs, [0, 10, 21], 2, 2, dst)             # recording 1 reaches past dst_rows
    assert err == 16 and (got[10:] == -7).all()
    rn.same_bits(got[:10], ok[:10])
    for row0 in ([-1, 10], [0, 15]):                                           # negative, reaching past dst_rows
        got, err, _ = rn.rasterize(ptr, pairs, [0, 10, 16], 2, 2, dst, dst_row0=row0)
        assert err == 16
    got, err, _ = rn.rasterize(ptr, pairs, [0, 10, 16], 2, 2, dst, point=[0, 1])
    assert err == 8 and (got[:16, 1] == -7).all()
    rn.same_bits(got[:, 0], ok[:, 0])
    got, err, _ = rn.rasterize(ptr, pairs, [0, 10, 16], 2, 2, dst, point=[-1, 0])
    assert err == 8 and (got[:16, 0] == -7).all()


def test_rows_overlap():
    from dcase2019_task4_amd.inference import rows_overlap
    assert not rows_overlap([0, 10, 16], [10, 6, 4]) and not rows_overlap([16, 0, 10], [4, 10, 6])
    assert rows_overlap([0, 9], [10, 3]) and rows_overlap([5, 0], [2, 6])
    assert not rows_overlap([3, 3], [0, 4])                                    # an empty recording shares nothing


def _cpu_sets():
    from dcase2019_task4_amd.longrec import WindowedFeatureSet
    from dcase2019_task4_amd.resident import ResidentFeatureSet
    rs = np.random.RandomState(0)
    lengths = [64, 64, 130, 200]
    feats = [np.abs(rs.standard_normal((n, 8))).astype(np.float32) for n in lengths]
    labels = [np.zeros((max(1, n // 8), 3), np.float32) for n in lengths]
    ws = WindowedFeatureSet.from_arrays(feats, labels, (2, 2), (1, 1), 64, [False, True], device="cpu", augment_type=None)
    clips = ResidentFeatureSet.from_arrays(feats[:2], labels[:2], (2,), (1,), frames=64, device="cpu", augment_type=None)
    bare = ResidentFeatureSet.from_arrays(feats[:2], None, None, None, frames=64, device="cpu", augment_type=None)
    return ws, clips, bare


def test_relabel_refuses_on_the_host_before_any_launch():
    from dcase2019_task4_amd import _lib
    ws, clips, bare = _cpu_sets()
    assert ws.label_rows_host.tolist() == [8, 8, 16, 25]
    table = (torch.zeros(2 * 3 + 1, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int32))
    f0 = [0, 16, 41]
    assert ws.check_relabel([2, 3], f0, 3)[1].tolist() == [16, 32]
    with pytest.raises(ValueError, match="named twice"):
        ws.relabel([2, 2], table, [0, 16, 32])
    with pytest.raises(ValueError, match=r"in \[0, 4\)"):
        ws.relabel([2, 4], table, f0)
    with pytest.raises(ValueError, match=r"in \[0, 4\)"):
        ws.relabel([-1, 3], table, f0)
    with pytest.raises(ValueError, match="recording 1 has 24 label frames, item 3 has label_rows = 25"):
        ws.relabel([2, 3], table, [0, 16, 40])
    with pytest.raises(ValueError, match="4 classes, the set's labels 3"):
        ws.relabel([2, 3], table, f0, nclass=4)
    with pytest.raises(ValueError, match="4 classes"):
        ws.relabel([2, 3], {"ev_ptr": table[0], "ev_pairs": table[1], "timeline": torch.zeros(41, 4)}, f0)
    with pytest.raises(ValueError, match="3 items for a table of 2"):
        ws.relabel([1, 2, 3], table, f0)
    with pytest.raises(ValueError, match="combine"):
        ws.relabel([2, 3], table, f0, combine="sum")
    with pytest.raises(_lib.SedError, match="GPU"):                            # every host check passed: there is no CPU path
        ws.relabel([2, 3], table, f0)
    # a resident set: every recording is T3 rows; a set without targets has nothing to relabel
    assert clips.check_relabel([1, 0], [0, 8, 16], 3)[1].tolist() == [8, 0]
    with pytest.raises(ValueError, match="recording 1 has 9 label frames, item 0 has T3 = 8"):
        clips.relabel([1, 0], table, [0, 8, 17])
    with pytest.raises(ValueError, match="no targets"):
        bare.relabel([0, 1], table, [0, 8, 16])
    before = ws.label_pool.clone()
    assert torch.equal(ws.label_pool, before)


def test_the_entry_refuses_bad_arguments_before_a_launch():
    """Host buffers only: every call returns SED_ERR_BAD_ARG before anything is launched."""
    from dcase2019_task4_amd import _lib
    l = _lib.lib()
    n_rec, NC, cap, rows = 2, 4, 6, 16
    ptr, pairs = torch.zeros(2 * n_rec * NC + 1, dtype=torch.int64), torch.zeros(cap, 2, dtype=torch.int32)
    value, point = torch.zeros(cap), torch.zeros(NC, dtype=torch.int32)
    f0, row0 = torch.tensor([0, 8, 16]), torch.tensor([0, 8])
    dst, err = torch.zeros(rows, NC), torch.full((1,), -7, dtype=torch.int32)
    base = dict(ptr=ptr, pairs=pairs, value=value, cap=cap, K=2, point=point, f0=f0, n_rec=n_rec, NC=NC, dst=dst, rows=rows,
                row0=row0, combine=0, err=err)

    def call(**kw):
        a = dict(base, **kw)
        p = lambda t: None if t is None else (t if isinstance(t, int) else _lib.ptr(t))
        return l.sed_events_rasterize(p(a["ptr"]), p(a["pairs"]), p(a["value"]), a["cap"], a["K"], p(a["point"]), p(a["f0"]),
                                      a["n_rec"], a["NC"], p(a["dst"]), a["rows"], p(a["row0"]), a["combine"], p(a["err"]), None)

    for name in ("ptr", "pairs", "f0", "dst", "err"):
        assert call(**{name: None}) == -1 and b"null" in l.sed_last_error(), name
    for kw in (dict(NC=0), dict(NC=17), dict(n_rec=0), dict(K=0), dict(K=4097), dict(K=4096, n_rec=4096), dict(cap=-1),
               dict(cap=1 << 31), dict(rows=-1), dict(rows=(1 << 31) // NC), dict(combine=2), dict(combine=-1)):
        assert call(**kw) == -1, kw
    assert call(pairs=pairs.data_ptr() + 4) == -1 and b"8-byte" in l.sed_last_error()
    for name in ("ptr", "pairs", "value", "point", "f0", "row0", "err"):
        assert call(dst=base[name]) == -1 and b"overlaps" in l.sed_last_error(), name
    assert int(err.item()) == -7 and not dst.any()

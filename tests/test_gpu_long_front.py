"""-m gpu test of the host front the four stitch entries share (sed_stitch_decode, sed_stitch_sweep, sed_stitch_weak,
sed_stitch_weak_backward): every entry refuses every bad geometry with SED_ERR_BAD_ARG and a message that begins with its own
name, before any launch - the outputs, the workspace and the error word keep their sentinels."""
import numpy as np
import pytest
import torch

from tests.long_util import SENT, _tables, _tile
from tests.test_gpu_long import _alternating_call
from tests.test_gpu_long_sweep import _alternating_sweep
from tests.test_gpu_long_weak import WeakCall
from tests.test_gpu_long_weak_bwd import BwdCall

pytestmark = pytest.mark.gpu

ENTRIES = ["sed_stitch_decode", "sed_stitch_sweep", "sed_stitch_weak", "sed_stitch_weak_backward"]
T3 = 8
BAD = [dict(T3=0), dict(T3=4097), dict(hop3=0), dict(hop3=T3 + 1), dict(weighting=2), dict(NC=0), dict(NC=17), dict(n_rec=0)]


@pytest.fixture(scope="module")
def calls():
    """One call object per entry on the smallest valid inputs: the two recordings of _alternating_sweep (L3 = 9 and tile + 3,
    T3 = hop3 = 8, NC = 3); the pooled entries take the posteriors as the attention too."""
    sweep, _, rec_frame0, p = _alternating_sweep()
    rec_win0, _ = _tables([9, _tile() + 3], T3, T3)
    return dict(zip(ENTRIES, (_alternating_call()[0], sweep, WeakCall(p, p, rec_win0, rec_frame0, T3, 0),
                              BwdCall(p, p, rec_win0, rec_frame0, T3, 0, np.ones((2, 3), np.float32)))))


def _stitch_untouched(call):
    torch.cuda.synchronize()
    return bool((call.ev_ptr == SENT).all() and (call.ev_pairs == SENT).all() and torch.isnan(call._tl).all()
                and (call.binary == 0xEE).all() and (call.ws == 0xFF).all()
                and int(call.err[0].item()) == 0 and int(call.err[1].item()) == SENT)


@pytest.mark.parametrize("bad", BAD, ids=lambda kw: "%s=%d" % next(iter(kw.items())))
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_refuses_a_bad_geometry_before_any_launch(calls, entry, bad):
    call = calls[entry]
    call.fill()
    good = {k: getattr(call, k) for k in bad}
    try:
        for k, v in bad.items():
            setattr(call, k, v)                                                  # (every launch() reads its geometry from the object)
        rc = call.launch()
    finally:
        for k, v in good.items():
            setattr(call, k, v)
    assert rc == -1                                                              # SED_ERR_BAD_ARG
    assert call.l.sed_last_error().startswith(entry.encode() + b": "), call.l.sed_last_error()
    assert call.untouched() if hasattr(call, "untouched") else _stitch_untouched(call)

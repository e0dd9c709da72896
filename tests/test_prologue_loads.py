"""CPU-side check of where the gfx950 compiler puts the prologue loads of the fp32 step's kernels (tools/serial_loads.py).

A load that sits behind its own `s_waitcnt vmcnt(0)` is one exposed memory round trip; kernels that run on the step's critical
chain beside an idle GPU pay each of them in full.  The source can say "issued back to back" and the compiled code can say
otherwise (the compiler sinks a load under the condition of its use, or behind a barrier when the memory is read-only), so the
compiled code is what is checked: the number of drain points in front of the first MFMA may not rise above what this tree
compiles to.  Compiles blk0.hip, bnglu.hip and conv.hip to assembly (about 40 s)."""
import os
import shutil
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

# kernel: (drain points before the first MFMA in the commit before the prologue rewrite, in this tree)
# The counts run over every path of the kernel: k_x_moments / k_x_moments_aux include the packing workgroups' path (3 of
# k_x_moments' 4; a moments workgroup has one drain point).  The dgrad k_conv_wino<TW,1> instantiations are not listed: their
# rewrite (5 -> 4) did not make the kernels shorter on the GPU and was taken out again (profiles/prologue_loads.md).
DRAINS = {
    "k_glu_pool_fwd": (15, 1),
    "k_glu_pool_bwd8": (7, 1),
    "k_x_moments": (8, 4),
    "k_x_moments_aux": (21, 18),
    "k_blk0_bwd_finalize": (10, 1),
}


@pytest.fixture(scope="module")
def streams():
    import serial_loads
    if not os.path.exists(serial_loads.HIPCC) or shutil.which("c++filt") is None:
        pytest.skip("no hipcc on this host: the check reads the gfx950 compiler's assembly")
    return serial_loads.analyze(["blk0.hip", "bnglu.hip", "conv.hip"])


@pytest.mark.parametrize("kernel", sorted(DRAINS))
def test_drain_points_before_the_first_mfma_do_not_come_back(streams, kernel):
    parent, now = DRAINS[kernel]
    assert now < parent
    loads, drains, _ = streams[kernel]
    print(f"{kernel}: {loads} loads, {drains} drain points (was {parent})")
    assert drains <= now, f"{kernel}: {drains} drain points in front of the first MFMA, this tree was committed with {now} (before: {parent})"


def test_the_five_tile_loads_of_the_patch_moments_are_issued_back_to_back(streams):
    """x_moments_body's tile is five float4 per thread - the kernel's only dwordx4 loads: no wait on the vector-memory
    counter may stand between the first and the fifth (each used to sit under its own exec mask with its own vmcnt(0)).
    (k_x_moments_aux shares the body, but the register allocation of its larger packing path leaves a wait between the third
    and the fourth load: it is held by its drain count only.)"""
    s = streams["k_x_moments"][2]
    idx = [i for i, t in enumerate(s) if t.startswith("global_load_dwordx4")]
    assert len(idx) == 5, len(idx)
    between = [t for t in s[idx[0]:idx[-1]] if t.startswith("s_waitcnt") and "vmcnt" in t]
    assert not between, between


def test_conv_wino_is_still_reported(streams):
    """The tool's figures for the dgrad Winograd kernels (not rewritten: see DRAINS) - printed, and held at the value they have."""
    for kernel in ("k_conv_wino<16,1>", "k_conv_wino<4,1>"):
        loads, drains, _ = streams[kernel]
        print(f"{kernel}: {loads} loads, {drains} drain points")
        assert drains <= 5, (kernel, drains)

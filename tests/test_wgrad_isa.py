"""What hipcc makes of k_wgrad's operand ring (csrc/ndp_kernels.hip: wgrad_loop), read in the gfx950 device assembly.

The ring is meant to refill every slot in place and to wait for one slot at a time; whether it does is decided by the
register allocator and the waitcnt insertion of the installed compiler, not by the source alone: the loop this one
replaced looked the same in the source and compiled to a second register set, 32 v_mov_b64, an accumulator round trip
through VGPRs and one s_waitcnt vmcnt(0) per pass.  So this test is tied to the installed hipcc (ROCm 7.2 here): with
another compiler a failure means "look at the loop again", not necessarily a wrong result.  Skipped without hipcc.

The assembly is produced once per module with the command line of scripts/isa.sh; scripts/wgrad_isa.py holds the parser
and prints the same census by hand.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import wgrad_isa  # noqa: E402

pytestmark = pytest.mark.skipif(wgrad_isa.hipcc() is None, reason="hipcc not installed")

PF = 8


@pytest.fixture(scope="module")
def loops(tmp_path_factory):
    return wgrad_isa.wgrad_loops(wgrad_isa.compile_asm(tmp_path_factory.mktemp("isa")))


@pytest.mark.parametrize("kernel", wgrad_isa.KERNELS)
def test_main_loops_refill_in_place_and_wait_by_count(loops, kernel):
    _, found = loops[kernel]
    for c in found:
        print(kernel, c)
    # 4 full loops (one per B-row map) of PF x 16 MFMAs, 2 skinny ones (SKINNY_B, SKINNY_A) of PF x 4
    assert sorted(c["mfma"] for c in found) == [4 * PF] * 2 + [16 * PF] * 4
    for c in found:
        assert c["vmcnt0"] == 0, c                                  # no drain inside the loop or on its back-edge
        assert c["vmcnt"] and min(c["vmcnt"]) >= 2 * (PF - 1) - 1, c  # each wait leaves the PF - 1 younger steps in flight
        assert c["accvgpr_read"] == 0 and c["accvgpr_write"] == 0, c  # accumulators stay where the MFMAs write them
        assert c["v_mov_b64"] == 0, c                               # no second register set copied over
        assert c["branches_inside"] == 0 and c["cond_branches"] == 1, c   # nothing decided inside but the back-edge
        assert c["vmem_loads"] == 2 * PF, c                         # one A and one B load per step


@pytest.mark.parametrize("kernel", wgrad_isa.KERNELS)
def test_no_scratch_and_two_workgroups_per_cu(loops, kernel):
    meta, _ = loops[kernel]
    print(kernel, meta)
    assert meta["ScratchSize"] == 0 and meta["private_segment_fixed_size"] == 0
    assert meta["TotalNumVgprs"] <= 256 and meta["next_free_vgpr"] <= 256   # VGPRs + AGPRs: two workgroups share a CU
    assert meta["Occupancy"] >= 2

"""CPU: what the larger read groups of the match-statistics kernel must leave alone on the host side.  The workspace of a
call does not depend on the group size: genie_find_smems_workspace_bytes returns what it returned before the launch plan
learned the 1536-position group (the figures below were taken from that build).  genie_launch_info needs an index that is
bound to a device, so the launch plan itself is checked in test_group_plan_gpu.py."""
import ctypes as C

import numpy as np
import pytest

WORKSPACE_BYTES = {
    (1, 1): 1792, (1, 100): 1792, (1, 150): 2048, (1, 250): 2048, (1, 255): 2048,
    (33, 1): 4352, (33, 100): 14592, (33, 150): 19456, (33, 250): 30208, (33, 255): 30208,
    (1000, 1): 89600, (1000, 100): 409600, (1000, 150): 553472, (1000, 250): 889344, (1000, 255): 889344,
    (1000000, 1): 88500480, (1000000, 100): 408500480, (1000000, 150): 552500480, (1000000, 250): 888500480,
    (1000000, 255): 888500480,
}


@pytest.fixture(scope="module")
def pkg():
    import genie_smem_amd as g
    g._native.build()
    g._native.lib()
    return g


def test_workspace_bytes_are_unchanged(pkg):
    lib = pkg._native.lib()
    got = {k: int(lib.genie_find_smems_workspace_bytes(*k)) for k in WORKSPACE_BYTES}
    assert got == WORKSPACE_BYTES


def test_launch_info_needs_a_device(pkg):
    """Why the plan's figures are asserted on the GPU: a host-only index has no launch."""
    ix = pkg.GenieIndex.build(np.random.default_rng(5).integers(0, 4, 500).astype(np.uint8), 8)
    g, b, l = C.c_int32(), C.c_int32(), C.c_int32()
    rc = pkg._native.lib().genie_launch_info(ix._h, pkg._native.MODES["bwa"], 150, C.byref(g), C.byref(b), C.byref(l))
    assert rc != 0
    ix.set_option(pkg._native.OPT_GROUP_POSITIONS, 768)      # the knob itself needs none
    ix.set_option(pkg._native.OPT_GROUP_POSITIONS, 0)

"""GPU (genie_launch_info needs an index bound to a device; nothing is launched): the launch plan of the match-statistics
kernel with groups of 1536 positions.  Where the compact table takes at most half an XCD's L2 the plan takes the larger group
only if three blocks still fit a CU's 160 KiB of LDS; a table that fills the L2 (4 MB: the 1 Mb reference's) keeps the
smaller one; GENIE_OPT_GROUP_POSITIONS = 768 gives the former, smaller layout; an index whose table exceeds the L2 (the 4-waves-per-SIMD build) keeps its groups of 768 positions, its grid and its block -- figures of
the build before the larger groups -- and needs no more LDS than it did."""
import pytest
import torch

import test_tuning_knobs_gpu as T

pytestmark = pytest.mark.gpu

LDS_CAP = 160 * 1024
# the 4-waves-per-SIMD build at 150 bases before the larger groups: two blocks per CU, 512 threads, 31 888 bytes of LDS
# (8 waves x 3 792 + 16 + 1 536); the slow list of a 750-position group is 512 entries now, 480 bytes less per wave
OLD_L2_MISS_LAUNCH = {"blocks_per_cu": 2, "block": 512, "lds_bytes": 31888}
NEW_L2_MISS_LDS = 31888 - 8 * 480


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import genie_smem_amd as g
    g._native.lib()
    return g


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_three_blocks_fit_the_lds_at_every_length(pkg):
    ix = T._build(pkg, "rand4096", 7, 0, "compact", 8, rmi=False)
    assert ix.search_kernel_name("bwa", 150).startswith("match_table_kernel<6, ")
    for max_len in (100, 150, 250, 255):
        info = ix.launch_info("bwa", max_len)
        assert 3 * info["lds_bytes"] <= LDS_CAP, (max_len, info)
        assert info["grid"] == 3 * _cus() and info["block"] == 512, (max_len, info)


def test_the_knob_gives_the_smaller_group(pkg):
    ix = T._build(pkg, "rand4096", 7, 0, "compact", 8, rmi=False)
    default = ix.launch_info("bwa", 150)
    assert default["lds_bytes"] == 8 * 5504 + 16 + 3072          # ten reads per group, a 512-entry slow list
    try:
        ix.set_option(pkg._native.OPT_GROUP_POSITIONS, 768)
        small = ix.launch_info("bwa", 150)
    finally:
        ix.set_option(pkg._native.OPT_GROUP_POSITIONS, 0)
    assert small["lds_bytes"] < default["lds_bytes"] and small["grid"] == default["grid"], (small, default)
    assert ix.launch_info("bwa", 150) == default


def test_a_table_that_fills_the_l2_keeps_the_smaller_group(pkg):
    ix = T._build(pkg, "rand4096", 7, 9, "compact", 8, rmi=False)          # 4^9 entries of 16 bytes = 4 MB
    assert ix.search_kernel_name("bwa", 150).startswith("match_table_kernel<6, ")
    info = ix.launch_info("bwa", 150)
    assert info == {"grid": 3 * _cus(), "block": 512, "lds_bytes": NEW_L2_MISS_LDS}, info
    try:
        ix.set_option(pkg._native.OPT_GROUP_POSITIONS, 768)
        assert ix.launch_info("bwa", 150) == info
        ix.set_option(pkg._native.OPT_GROUP_POSITIONS, 1536)                # the knob still reaches the larger group
        assert ix.launch_info("bwa", 150)["lds_bytes"] == 8 * 5504 + 16 + 3072
    finally:
        ix.set_option(pkg._native.OPT_GROUP_POSITIONS, 0)


def test_a_table_beyond_the_l2_keeps_its_launch(pkg):
    ix = T._build(pkg, "rand4096", 7, 11, "compact", 8, rmi=False)
    assert ix.search_kernel_name("bwa", 150).startswith("match_table_kernel<4, ")
    info = ix.launch_info("bwa", 150)
    assert info["grid"] == OLD_L2_MISS_LAUNCH["blocks_per_cu"] * _cus() and info["block"] == OLD_L2_MISS_LAUNCH["block"], info
    assert info["lds_bytes"] == NEW_L2_MISS_LDS <= OLD_L2_MISS_LAUNCH["lds_bytes"], info
    try:                                                          # the default is the 768-position group
        ix.set_option(pkg._native.OPT_GROUP_POSITIONS, 768)
        assert ix.launch_info("bwa", 150) == info
    finally:
        ix.set_option(pkg._native.OPT_GROUP_POSITIONS, 0)

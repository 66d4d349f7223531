"""CPU-only pin of the public workspace and scratch sizes.  Callers (bench.py among them) allocate by these numbers, and
each launch cuts the caller's buffer by the same layout, so the values below -- recorded before the layouts were
rewritten as one bump carver each -- must not move."""
import pytest

MAX_LENS = [0, 150, 255, 256, 8192]
TOTALS = [0, 10**4, 10**8]
SCRATCH_N = [0, 1, 1000, 10**6, 10**7]

# N -> bytes at each of MAX_LENS
FIND = {
    0: [512, 512, 512, 512, 512],
    1: [1792, 2048, 2048, 3072, 54528],
    1000: [89600, 553472, 889344, 1705216, 53289216],
    1000000: [88500480, 552500480, 888500480, 1704500480, 53288500480],
}
SPLIT = {
    0: [4352, 4608, 4608, 5632, 65024],
    1: [4608, 4864, 4864, 5888, 65280],
    1000: [144128, 751872, 1183744, 1999616, 61519616],
    1000000: [141501696, 749501696, 1181501696, 1997501696, 61517501696],
}
# N -> bytes at each of TOTALS (the same for every max_len)
LONG = {
    0: [1536, 174848, 1731251200],
    1: [2048, 175360, 1731251712],
    1000: [49152, 223232, 1731299584],
    1000000: [48009216, 48182528, 1779258880],
}
# at each of SCRATCH_N
COMPACT = [32, 40, 40, 7848, 78160]
LOCATE = [512, 768, 4608, 4008192, 40078592]


@pytest.fixture(scope="module")
def lib():
    import genie_smem_amd as g
    g._native.build()
    return g._native.lib()


def test_find_smems_workspace_bytes(lib):
    for n, want in FIND.items():
        assert [lib.genie_find_smems_workspace_bytes(n, m) for m in MAX_LENS] == want, n


def test_split_workspace_bytes(lib):
    for n, want in SPLIT.items():
        assert [lib.genie_find_smems_split_workspace_bytes(n, m) for m in MAX_LENS] == want, n


def test_long_workspace_bytes(lib):
    for n, want in LONG.items():
        for m in MAX_LENS:
            assert [lib.genie_find_smems_long_workspace_bytes(n, t, m) for t in TOTALS] == want, (n, m)


def test_compact_and_locate_tmp_bytes(lib):
    assert [lib.genie_compact_tmp_bytes(s) for s in SCRATCH_N] == COMPACT
    assert [lib.genie_locate_tmp_bytes(s) for s in SCRATCH_N] == LOCATE

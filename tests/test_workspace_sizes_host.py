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
# The calls with a step (contig-exact, min_occ), recorded before their sizing became one function: N -> for each of the
# flags 0 .. 3 (BOTH_STRANDS = 1, SPLIT_BREAKS = 2) the bytes at each of TOTALS; the same for every max_len and n_contigs
STEP_FLAGS = [0, 1, 2, 3]
STEP_MAX_LENS = [0, 150, 8192]
MATCH_STATS_CONTIGS = {
    0: [[9472, 132096, 1227352832], [10240, 255488, 2454697472], [11520, 153600, 1433677568], [11520, 297216, 2867344384]],
    1: [[9728, 132352, 1227353088], [10240, 255488, 2454697472], [11520, 153600, 1433677568], [11520, 297216, 2867344384]],
    1000: [[43008, 166400, 1227387136], [109568, 355328, 2454797312], [80128, 223744, 1433746688], [150528, 438016, 2867483904]],
    1000000: [[34017024, 34139648, 1261360640], [100025344, 100270592, 2554712576], [70017792, 70161408, 1503685376], [140025856, 140312832, 3007360000]],
}
FIND_SMEMS_CONTIGS = {
    0: [[10240, 263680, 2533603328], [11264, 517888, 5067198464], [12800, 294144, 2827428352], [12800, 577280, 5654845184]],
    1: [[10752, 264192, 2533603840], [11264, 517888, 5067198464], [12800, 294144, 2827428352], [12800, 577280, 5654845184]],
    1000: [[63488, 318208, 2533657856], [150272, 657408, 5067337984], [108800, 392704, 2827525376], [207360, 774144, 5655040768]],
    1000000: [[54017792, 54271232, 2587611136], [140026112, 140532736, 5207213312], [98018816, 98301696, 2925436160], [196026880, 196591872, 5850860800]],
}
MATCH_STATS_MIN_OCC = {
    0: [[1280, 43776, 426563584], [2048, 87296, 853126912], [3328, 64768, 626735872], [3328, 127744, 1253468928]],
    1: [[1536, 44032, 426563840], [2048, 87296, 853126912], [3328, 64768, 626735872], [3328, 127744, 1253468928]],
    1000: [[33024, 76032, 426595840], [97536, 183040, 853222656], [70144, 132864, 626802944], [138496, 264448, 1253604608]],
    1000000: [[32040192, 32082688, 458602496], [96079616, 96164864, 949204480], [68040960, 68103680, 694774784], [136080128, 136205824, 1389547264]],
}
FIND_SMEMS_MIN_OCC = {
    0: [[2048, 175360, 1732814080], [3072, 349696, 3465627904], [4608, 205312, 2020486656], [4608, 407808, 4040969728]],
    1: [[2560, 175872, 1732814592], [3072, 349696, 3465627904], [4608, 205312, 2020486656], [4608, 407808, 4040969728]],
    1000: [[53504, 227840, 1732866560], [138240, 485120, 3465763328], [98816, 301824, 2020581632], [195328, 600576, 4041161472]],
    1000000: [[52040960, 52214272, 1784852992], [136080384, 136427008, 3601705216], [96041984, 96243968, 2116525568], [192081152, 192484864, 4233048064]],
}
# at each of SCRATCH_N
COMPACT = [32, 40, 40, 7848, 78160]
LOCATE = [512, 768, 4608, 4008192, 40078592]
# The ingestion calls, recorded before their kernels were put on shared tile pieces: at each of INGEST_BYTES (text_bytes or
# n_given) the bytes at each of INGEST_COUNTS (cap_reads or n_records)
INGEST_BYTES = [0, 1, 4095, 4096, 4097, 10**8]
INGEST_COUNTS = [0, 1, 10**6]
INGEST = {
    "reads_from_text": [[1536] * 3] * 5 + [[781824, 781824, 789504]],
    "reads_from_fasta": [[1536] * 3] * 5 + [[1172224] * 3],
    "reference_segments": [[1024] * 3] * 5 + [[781568] * 3],
}


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


@pytest.mark.parametrize("name, want, contigs", [
    ("match_stats_contigs", MATCH_STATS_CONTIGS, (1, 25)),
    ("find_smems_contigs", FIND_SMEMS_CONTIGS, (1, 25)),
    ("match_stats_min_occ", MATCH_STATS_MIN_OCC, None),
    ("find_smems_min_occ", FIND_SMEMS_MIN_OCC, None),
])
def test_step_call_workspace_bytes(lib, name, want, contigs):
    size = getattr(lib, f"genie_{name}_workspace_bytes")
    for n, rows in want.items():
        for flags, row in zip(STEP_FLAGS, rows):
            for m in STEP_MAX_LENS:
                for tail in ([(c,) for c in contigs] if contigs else [()]):
                    assert [size(n, t, m, flags, *tail) for t in TOTALS] == row, (n, flags, m, tail)
            assert all(b % 256 == 0 for b in row), (n, flags)      # what the tests' drivers assert of every call


def test_compact_and_locate_tmp_bytes(lib):
    assert [lib.genie_compact_tmp_bytes(s) for s in SCRATCH_N] == COMPACT
    assert [lib.genie_locate_tmp_bytes(s) for s in SCRATCH_N] == LOCATE


@pytest.mark.parametrize("name", list(INGEST))
def test_ingest_tmp_bytes(lib, name):
    size = getattr(lib, f"genie_{name}_tmp_bytes")
    assert [[size(b, c) for c in INGEST_COUNTS] for b in INGEST_BYTES] == INGEST[name]

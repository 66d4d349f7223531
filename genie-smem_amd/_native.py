"""ctypes binding of the C-ABI library (include/genie_smem.h -> libgenie_smem.so).

There is no CPU fallback: if the library is missing or a call fails this module raises.
torch is imported first on purpose -- PyTorch-ROCm ships its own libamdhip64.so.7; loading it
first makes our library resolve the same HIP runtime, so torch tensors' device pointers and
streams are valid inside our launches.
"""
import ctypes as C
import os
import subprocess

import torch  # noqa: F401  (must precede the CDLL below, see docstring)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libgenie_smem.so")
CSRC = os.path.join(_PKG, "csrc")

ABI_VERSION = 2
HEADER_BYTES = 512
MAX_K = 16
MAX_READ_LEN = 8192
MODE_BWA, MODE_LUT, MODE_RMI = 0, 1, 2
MODES = {"bwa": MODE_BWA, "lut": MODE_LUT, "rmi": MODE_RMI}
IMAGE_NO_SEED_TABLE = 1
TABLE_WIDE, TABLE_COMPACT = 1 << 8, 2 << 8        # genie_index_create_ex: ORed into table_bits
OPT_SEARCH_ALL = 2
OPT_GROUP_POSITIONS = 4
OPT_SEARCH_ONLY = 5
OPT_SEARCH_BLOCKS_PER_CU = 6
OPT_SEARCH_STAGES_OFF = 7
OPT_SCHEDULING = 8
READ_OK, READ_BAD_BASE, READ_TOO_SHORT, READ_ABSENT_BASE, READ_OVERFLOW = 0, 1, 2, 3, 4
READS_BOTH_STRANDS, READS_SPLIT_BREAKS = 1, 2       # flags of genie_find_smems_long_ex, genie_match_stats, genie_exact_match, genie_find_mems
TEXT_LINES, TEXT_FASTQ = 0, 1                       # formats of genie_reads_from_text
TEXT_FORMATS = {"lines": TEXT_LINES, "fastq": TEXT_FASTQ}
TEXT_PARTIAL = 1                                    # its flag
SEG_POSITIONS, SEG_HITS = 0, 1                      # forms of genie_segment_coords
SEG_FORMS = {"positions": SEG_POSITIONS, "hits": SEG_HITS}
SELECT_LANE_MAX, SELECT_TILE = 8, 512               # genie_select_alignments: one lane per read up to the first, LDS state up to the second
PAIR_LANE_MAX, PAIR_TILE = 64, 256                  # genie_pair_alignments: one lane per pair up to the first (combinations), LDS records per mate
PAIR_ORIENT = {"fr": 1, "rf": 2, "same": 4, "any": 7}
ISIZE_LDS_BINS = 4096                               # genie_insert_size_stats: spans below it are counted in LDS
ISIZE_OUTLIER_IQR, ISIZE_WINDOW_IQR, ISIZE_WINDOW_STD = 2, 3, 4   # its multipliers (BWA-MEM's)
WINDOW_MAX, WINDOW_MAX_ROWS = 65536, 2048           # genie_window_mems: bases of a window, rows of a searched unit (sized to LDS)
WINDOW_SEARCHED, WINDOW_ROW_CAP, WINDOW_TOO_LONG = 1, 2, 4   # its status values
SAM_NM, SAM_AS, SAM_MD, SAM_MC, SAM_MQ = 1, 2, 4, 8, 16      # genie_sam_text: the tags, written in this order
SAM_NO_SEQ = 1                                      # its flag

# every symbol include/genie_smem.h declares (tests check the library exports all of them)
SYMBOLS = [
    "genie_abi_version", "genie_index_create", "genie_index_create_from_sa", "genie_index_create_ex", "genie_index_set_rmi",
    "genie_index_info", "genie_index_suffix_array", "genie_index_lut_arrays", "genie_index_blob_bytes",
    "genie_index_serialize", "genie_index_image_bytes", "genie_index_serialize_image", "genie_index_open", "genie_index_validate", "genie_index_to_device", "genie_index_destroy",
    "genie_index_device_image_bound", "genie_index_device_build_tmp_bytes", "genie_index_create_device",
    "genie_sa_interval", "genie_seed_lookup", "genie_find_smems", "genie_find_smems_csr", "genie_find_smems_packed", "genie_find_smems_packed6", "genie_find_smems_workspace_bytes", "genie_find_smems_workspace_rows",
    "genie_find_smems_split", "genie_find_smems_split_workspace_bytes",
    "genie_find_smems_long", "genie_find_smems_long_workspace_bytes",
    "genie_find_smems_long_ex", "genie_find_smems_long_ex_workspace_bytes",
    "genie_find_smems_both", "genie_find_smems_both_workspace_bytes",
    "genie_match_stats", "genie_match_stats_workspace_bytes",
    "genie_exact_match", "genie_exact_match_workspace_bytes",
    "genie_find_mems", "genie_find_mems_workspace_bytes",
    "genie_contigs_validate", "genie_find_mems_contigs", "genie_find_mems_contigs_workspace_bytes",
    "genie_locate_contigs", "genie_locate_contigs_tmp_bytes", "genie_contig_coords",
    "genie_match_stats_contigs", "genie_match_stats_contigs_workspace_bytes",
    "genie_find_smems_contigs", "genie_find_smems_contigs_workspace_bytes",
    "genie_match_stats_min_occ", "genie_match_stats_min_occ_workspace_bytes",
    "genie_find_smems_min_occ", "genie_find_smems_min_occ_workspace_bytes",
    "genie_chain_mems", "genie_chain_mems_workspace_bytes",
    "genie_align_chains", "genie_align_chains_workspace_bytes",
    "genie_chain_cigars", "genie_chain_cigars_workspace_bytes",
    "genie_select_alignments", "genie_select_alignments_workspace_bytes",
    "genie_pair_alignments", "genie_pair_alignments_workspace_bytes",
    "genie_insert_size_stats", "genie_insert_size_stats_workspace_bytes",
    "genie_rescue_windows", "genie_rescue_windows_workspace_bytes",
    "genie_window_mems", "genie_window_mems_workspace_bytes",
    "genie_sam_text", "genie_sam_text_workspace_bytes",
    "genie_bam_records", "genie_bam_records_workspace_bytes",
    "genie_reads_from_text", "genie_reads_from_text_tmp_bytes",
    "genie_reads_from_fasta", "genie_reads_from_fasta_tmp_bytes",
    "genie_reference_segments", "genie_reference_segments_tmp_bytes", "genie_segment_coords",
    "genie_compact_tmp_bytes",
    "genie_compact_smems", "genie_locate_tmp_bytes", "genie_locate", "genie_index_train_rmi", "genie_index_rmi_models", "genie_launch_info", "genie_search_kernel_name", "genie_index_set_option", "genie_index_set_stage_events", "genie_strerror", "genie_last_hip_error",
]


class GenieInfo(C.Structure):
    _fields_ = [("n", C.c_int64), ("K", C.c_int32), ("dir_bits", C.c_int32), ("lut_keys", C.c_int64),
                ("lut_slots", C.c_int64), ("rmi_levels", C.c_int32), ("has_host", C.c_int32),
                ("has_device", C.c_int32), ("device", C.c_int32), ("blob_bytes", C.c_int64)]


class GenieError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        msg = lib().genie_strerror(status).decode()
        if status == -5:
            msg += " [" + lib().genie_last_hip_error().decode() + "]"
        super().__init__(f"{where}: {msg} (status {status})")


def build(force=False):
    """Compile libgenie_smem.so for gfx950 with hipcc (csrc/Makefile), in-tree."""
    srcs = [os.path.join(CSRC, f) for f in ("kernels.hip", "index_build.hip", "short_read_kernel.inc", "match_table_kernel.inc", "match_table_body.inc", "match_table_long_body.inc", "split_reads.inc", "long_reads.inc", "long_units.inc", "lu_seg_body.inc", "exact_match.inc", "contigs.inc", "fwd_step.inc", "contig_stats.inc", "min_occ.inc", "mems.inc", "chains.inc", "align.inc", "cigars.inc", "select.inc", "pairs.inc", "insert_size.inc", "windows.inc", "sam_text.inc", "bam_records.inc", "ingest_tiles.inc", "text_reads.inc", "fasta_reads.inc", "segments.inc", "capi.cpp", "index_host.cpp", "genie_internal.h", "Makefile")]
    srcs.append(os.path.join(os.path.dirname(_PKG), "include", "genie_smem.h"))
    newest = max(os.path.getmtime(s) for s in srcs)
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < newest:
        subprocess.check_call(["make", "-s", "-C", CSRC] + (["-B"] if force else []))
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP library has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C genie-smem_amd/csrc`). "
            "There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    u8p, i32p, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    vpp = C.POINTER(C.c_void_p)
    sig = {
        "genie_abi_version": (C.c_int, []),
        "genie_index_create": (C.c_int, [u8p, i64, i32, i32, vpp]),
        "genie_index_create_from_sa": (C.c_int, [u8p, i64, i32p, i32, i32, vpp]),
        "genie_index_create_ex": (C.c_int, [u8p, i64, i32p, i32, i32, i32, vpp]),
        "genie_index_set_rmi": (C.c_int, [vp, i32, i32p, i32p, dp, dp]),
        "genie_index_info": (C.c_int, [vp, C.POINTER(GenieInfo)]),
        "genie_index_suffix_array": (i32p, [vp]),
        "genie_index_lut_arrays": (C.c_int, [vp, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(i32p), C.POINTER(i32p)]),
        "genie_index_blob_bytes": (i64, [vp]),
        "genie_index_serialize": (C.c_int, [vp, vp, i64]),
        "genie_index_image_bytes": (i64, [vp, i32]),
        "genie_index_serialize_image": (C.c_int, [vp, i32, vp, i64]),
        "genie_index_open": (C.c_int, [vp, vp, i64, i32, vpp]),
        "genie_index_validate": (C.c_int, [vp, C.POINTER(C.c_uint32), vp]),
        "genie_index_to_device": (C.c_int, [vp, i32]),
        "genie_index_destroy": (None, [vp]),
        "genie_index_device_image_bound": (i64, [i64, i32, i32, i32]),
        "genie_index_device_build_tmp_bytes": (i64, [i64, i32, i32, i32]),
        "genie_index_create_device": (C.c_int, [vp, i64, i32, i32, i32, i32, vp, i64, C.POINTER(C.c_int64), vp, i64, i32, vp,
                                                vpp]),
        "genie_sa_interval": (C.c_int, [vp, vp, vp, i64, i32, i32, vp, vp]),
        "genie_seed_lookup": (C.c_int, [vp, i32, vp, i64, vp, vp, vp]),
        "genie_find_smems": (C.c_int, [vp, i32, vp, vp, i64, i32, i32, i32, vp, vp, i32, vp, vp, i64, vp]),
        "genie_find_smems_csr": (C.c_int, [vp, i32, vp, vp, i64, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp]),
        "genie_find_smems_packed": (C.c_int, [vp, i32, vp, vp, i64, i32, i32, i32, vp, vp, vp, i64, vp, vp, i64, vp, i64, vp]),
        "genie_find_smems_packed6": (C.c_int, [vp, i32, vp, vp, i64, i32, i32, i32, vp, vp, vp, i64, vp, vp, i64, vp, i64, vp]),
        "genie_find_smems_workspace_bytes": (i64, [i64, i32]),
        "genie_find_smems_workspace_rows": (C.c_int, [i32, i32p]),
        "genie_find_smems_split": (C.c_int, [vp, vp, vp, i64, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp]),
        "genie_find_smems_split_workspace_bytes": (i64, [i64, i32]),
        "genie_find_smems_long": (C.c_int, [vp, i32, vp, vp, i64, i64, i64, i32, vp, vp, i64, vp, vp, i64, vp]),
        "genie_find_smems_long_workspace_bytes": (i64, [i64, i64, i64]),
        "genie_find_smems_long_ex": (C.c_int, [vp, i32, i32, vp, vp, i64, i64, i64, i32, vp, vp, i64, vp, vp, i64, vp]),
        "genie_find_smems_long_ex_workspace_bytes": (i64, [i64, i64, i64, i32]),
        "genie_find_smems_both": (C.c_int, [vp, i32, vp, vp, i64, i32, i32, i32, vp, vp, i64, vp, vp, i64, vp]),
        "genie_find_smems_both_workspace_bytes": (i64, [i64, i32]),
        "genie_match_stats": (C.c_int, [vp, i32, vp, vp, i64, i64, i64, vp, vp, vp, vp, i64, vp]),
        "genie_match_stats_workspace_bytes": (i64, [i64, i64, i64, i32]),
        "genie_exact_match": (C.c_int, [vp, i32, vp, vp, i64, i64, i64, vp, vp, vp, vp, i64, vp]),
        "genie_exact_match_workspace_bytes": (i64, [i64, i64, i64, i32]),
        "genie_find_mems": (C.c_int, [vp, i32, vp, vp, i64, i64, i64, i32, i32, vp, vp, i64, vp, vp, vp, i64, vp]),
        "genie_find_mems_workspace_bytes": (i64, [i64, i64, i64, i32]),
        "genie_contigs_validate": (C.c_int, [vp, vp, i64, vp]),
        "genie_find_mems_contigs": (C.c_int, [vp, vp, i64, i32, vp, vp, i64, i64, i64, i32, i32, vp, vp, i64, vp, vp, vp, i64, vp]),
        "genie_find_mems_contigs_workspace_bytes": (i64, [i64, i64, i64, i32, i64]),
        "genie_locate_contigs_tmp_bytes": (i64, [i64]),
        "genie_locate_contigs": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, i64, vp]),
        "genie_contig_coords": (C.c_int, [vp, vp, i64, vp, i32, i64, vp, vp]),
        "genie_match_stats_contigs": (C.c_int, [vp, vp, i64, i32, vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, i64, vp]),
        "genie_match_stats_contigs_workspace_bytes": (i64, [i64, i64, i64, i32, i64]),
        "genie_find_smems_contigs": (C.c_int, [vp, vp, i64, i32, i32, vp, vp, i64, i64, i64, i32, vp, vp, i64, vp, vp, vp, i64, vp]),
        "genie_find_smems_contigs_workspace_bytes": (i64, [i64, i64, i64, i32, i64]),
        "genie_match_stats_min_occ": (C.c_int, [vp, i32, i32, vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, i64, vp]),
        "genie_match_stats_min_occ_workspace_bytes": (i64, [i64, i64, i64, i32]),
        "genie_find_smems_min_occ": (C.c_int, [vp, i32, i32, vp, vp, i64, i64, i64, i32, i32, vp, vp, i64, vp, vp, vp, i64, vp]),
        "genie_find_smems_min_occ_workspace_bytes": (i64, [i64, i64, i64, i32]),
        "genie_chain_mems_workspace_bytes": (i64, [i64, i64, i64]),
        "genie_chain_mems": (C.c_int, [vp, vp, i64, vp, vp, i64, i64, i32, i32, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp]),
        "genie_align_chains_workspace_bytes": (i64, [i64, i64]),
        "genie_align_chains": (C.c_int, [vp, vp, i64, i32, vp, vp, i64, i64, i64, vp, vp, i64, i64, vp, vp, vp, vp, i64, i32, i32, i32, i32,
                                         i32, i32, i32, vp, vp, vp, i64, vp]),
        "genie_chain_cigars_workspace_bytes": (i64, [i64, i64, i64, i64]),
        "genie_chain_cigars": (C.c_int, [vp, vp, i64, i32, vp, vp, i64, i64, i64, vp, vp, i64, i64, vp, vp, vp, vp, i64, i32, i32, i32, i32,
                                         i32, i32, i32, vp, vp, i64, vp, vp, i64, vp, vp, vp, i64, vp, i64, vp]),
        "genie_select_alignments_workspace_bytes": (i64, [i64, i64]),
        "genie_select_alignments": (C.c_int, [vp, vp, i64, i32, vp, i64, vp, i64, vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, vp, vp,
                                              i64, vp, vp, vp, i64, vp]),
        "genie_pair_alignments_workspace_bytes": (i64, [i64, i64]),
        "genie_pair_alignments": (C.c_int, [vp, i64, vp, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i64, vp]),
        "genie_insert_size_stats_workspace_bytes": (i64, [i64, i32]),
        "genie_insert_size_stats": (C.c_int, [vp, i64, vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, i64, vp]),
        "genie_rescue_windows_workspace_bytes": (i64, [i64]),
        "genie_rescue_windows": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, i64, vp, i32, i32, i32, vp, vp, vp, i64, vp]),
        "genie_window_mems_workspace_bytes": (i64, [i64]),
        "genie_window_mems": (C.c_int, [vp, i32, vp, vp, i64, i64, i64, i64, vp, i32, vp, vp, i64, vp, vp, i64, vp, vp, vp, i64, vp]),
        "genie_sam_text_workspace_bytes": (i64, [i64, i64]),
        "genie_sam_text": (C.c_int, [vp, vp, i64, vp, vp, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, i32, i32,
                                     vp, vp, i64, vp, vp, i64, vp]),
        "genie_bam_records_workspace_bytes": (i64, [i64, i64]),
        "genie_bam_records": (C.c_int, [vp, vp, i64, vp, vp, i64, i64, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp, vp, i64, vp, vp, i64, i32, i32,
                                        vp, vp, i64, vp, vp, i64, vp]),
        "genie_reads_from_text_tmp_bytes": (i64, [i64, i64]),
        "genie_reads_from_text": (C.c_int, [vp, i64, i32, i32, vp, vp, i64, vp, i64, vp, vp, i64, vp]),
        "genie_reads_from_fasta_tmp_bytes": (i64, [i64, i64]),
        "genie_reads_from_fasta": (C.c_int, [vp, i64, i32, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp]),
        "genie_reference_segments_tmp_bytes": (i64, [i64, i64]),
        "genie_reference_segments": (C.c_int, [vp, i64, vp, i64, vp, i64, vp, vp, vp, i64, vp, vp, i64, vp]),
        "genie_segment_coords": (C.c_int, [vp, vp, vp, vp, i64, i32, vp, i32, i64, vp, vp]),
        "genie_compact_tmp_bytes": (i64, [i64]),
        "genie_compact_smems": (C.c_int, [vp, vp, i64, i32, vp, vp, i64, vp, vp]),
        "genie_index_train_rmi": (C.c_int, [vp, i32, vp, vp, vp]),
        "genie_index_rmi_models": (C.c_int, [vp, vp, vp, vp]),
        "genie_locate_tmp_bytes": (i64, [i64]),
        "genie_locate": (C.c_int, [vp, vp, i32, i64, vp, vp, i64, vp, i64, vp]),
        "genie_launch_info": (C.c_int, [vp, i32, i32, i32p, i32p, i32p]),
        "genie_search_kernel_name": (C.c_int, [vp, i32, i32, C.c_char_p, i32]),
        "genie_index_set_option": (C.c_int, [vp, i32, i32]),
        "genie_index_set_stage_events": (C.c_int, [vp, vp, vp]),
        "genie_strerror": (C.c_char_p, [C.c_int]),
        "genie_last_hip_error": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.genie_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libgenie_smem.so: ABI version {L.genie_abi_version()}, this binding is for {ABI_VERSION} "
                           "(rebuild: make -C genie-smem_amd/csrc)")
    _lib = L
    return L


def check(status, where):
    if status != 0:
        raise GenieError(status, where)

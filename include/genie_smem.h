/*
 * genie_smem.h -- C ABI of the MI355X-native batched SMEM finder (libgenie_smem.so).
 *
 * This is the drop-in boundary for the one hot path of jgkellymit/GENIE-SMEM: seed lookup,
 * suffix-array interval search and the SMEM extension loop.  The reference has no FFI (it is
 * in-process Python), so each entry point names the reference method it replaces; the Python
 * classes in genie-smem_amd/ bind these with ctypes and re-expose the reference's own method
 * names (see INTEGRATION.md for the binding a maintainer of the reference would add).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in any signature (`stream` is a
 *     hipStream_t passed as void*, 0 = the null stream);
 *   - pointers named d_* are DEVICE pointers owned by the caller (e.g. torch tensors);
 *     everything else is host memory;
 *   - bases are codes 0..3 in the sorted order of the reference alphabet (ACGT -> 0..3, the
 *     map of LUT.convert_seq_to_num, reference SMEM/LUT.py:37-48);
 *   - suffix-array rows: n+1 rows, row 0 is the '$' suffix; intervals are 0-based inclusive
 *     [lo, hi] exactly as ExactMatch.exact_match_back_prop returns them (SMEM/ExactMatch.py:151);
 *     an absent pattern is (-1, -1) where the reference returns the int -1;
 *   - every function returns 0 (GENIE_OK) or a negative genie_status; none throws.  (One positive code exists,
 *     GENIE_W_SEARCH_ONLY, returned only while the timing knob GENIE_OPT_SEARCH_ONLY is set.)
 *   - an index handle is immutable once opened on a device: any number of concurrent calls on
 *     distinct streams may share it.
 */
#ifndef GENIE_SMEM_H
#define GENIE_SMEM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GENIE_ABI_VERSION 2      /* 2: GENIE_W_SEARCH_ONLY, option codes renumbered since 1, workspace layout, image version */
#define GENIE_HEADER_BYTES 512      /* fixed-size header at the start of a serialized index */
#define GENIE_MAX_K 16              /* K-mer codes are 32-bit (2 bits per base) */
#define GENIE_MAX_DIR_BITS 7        /* P: prefix directory has 4^P + 1 entries (64 KB: genie_sa_interval stages it in LDS) */
#define GENIE_MAX_READ_LEN 8192     /* per-read scratch lives in LDS */
#define GENIE_MAX_RMI_LEVELS 4

typedef enum genie_status {
    GENIE_OK = 0,
    GENIE_E_INVALID = -1,      /* bad argument (null pointer, negative size, K out of range ...) */
    GENIE_E_ALPHABET = -2,     /* a base code > 3 in the reference */
    GENIE_E_NOMEM = -3,
    GENIE_E_NO_DEVICE = -4,    /* index has no device image (call genie_index_open / _to_device) */
    GENIE_E_HIP = -5,          /* HIP runtime error; see genie_last_hip_error() */
    GENIE_E_TOO_LONG = -6,     /* read/pattern longer than GENIE_MAX_READ_LEN, or a batch beyond what one launch covers
                                  ("Batch sizes" at genie_find_smems_long) */
    GENIE_E_NO_MODEL = -7,     /* RMI mode requested but no model was set */
    GENIE_E_BAD_BLOB = -8,     /* serialized index: wrong magic / version / size */
    GENIE_E_NO_LUT = -9,       /* LUT mode requested but the index was built with K = 0, or the image has no seed table */
    GENIE_E_CAPACITY = -10,    /* output buffer too small (compaction) */
    GENIE_W_SEARCH_ONLY = 1    /* GENIE_OPT_SEARCH_ONLY is set: only the match-statistics kernel was launched;
                                  counts / offsets / rows were NOT written */
} genie_status;

/* Per-read status written by genie_find_smems into d_status (0 = ok).  They mirror how the
 * reference fails on the same input (SURVEY.md section 8a "quirks"). */
enum {
    GENIE_READ_OK = 0,
    GENIE_READ_BAD_BASE = 1,   /* code > 3: reference raises KeyError (ExactMatch.py:139, LUT.py:47) */
    GENIE_READ_TOO_SHORT = 2,  /* len < K in LUT/RMI mode: reference mis-encodes (SMEM.py:26-28) */
    GENIE_READ_ABSENT_BASE = 3,/* a base that never occurs in the reference: reference raises
                                  KeyError('') (SMEM.py:39) or never terminates (SMEM.py:465,484) */
    GENIE_READ_OVERFLOW = 4    /* more SMEMs than `cap` slots; d_counts holds the true count */
};

/* SMEM traversal selector == which reference method is replaced. */
enum {
    GENIE_MODE_BWA = 0,        /* SMEM.get_SMEMS        (SMEM/SMEM.py:456-467) */
    GENIE_MODE_LUT = 1,        /* SMEM.get_smems_lut    (SMEM/SMEM.py:20-192)  */
    GENIE_MODE_RMI = 2         /* SMEM.get_smems_rmi    (SMEM/SMEM.py:206-384) */
};

typedef struct genie_index genie_index;

typedef struct genie_info {
    int64_t n;                 /* reference length in bases (without '$') */
    int32_t K;                 /* LUT / RMI key size (lut_size, prediction_size); 0 = none */
    int32_t dir_bits;          /* P */
    int64_t lut_keys;          /* distinct K-mers (len(lut.lut) in the reference) */
    int64_t lut_slots;         /* device hash-table slots */
    int32_t rmi_levels;        /* 0 = no model */
    int32_t has_host;          /* host arrays present (built here, not attached from a blob) */
    int32_t has_device;        /* device image bound */
    int32_t device;            /* HIP device ordinal of the image, -1 if none */
    int64_t blob_bytes;        /* size of the serialized / device image */
} genie_info;

/* ---------------------------------------------------------------------------------------
 * Index construction (host).  Replaces ExactMatch.create_fm_index + LUT.generate_lut
 * (SMEM/ExactMatch.py:22-33, SMEM/LUT.py:15-35): builds the suffix array of ref+"$", the
 * 2-bit packed reference, the P-mer prefix directory and (K > 0) the K-mer table.
 * No FM Occ/BWT is built: suffix-array bound search gives the same intervals (tests pin this).
 * ------------------------------------------------------------------------------------- */
int genie_index_create(const uint8_t *codes, int64_t n, int32_t K, int32_t dir_bits, genie_index **out);

/* Same, but adopt a suffix array supplied by the caller in the reference's JSON convention
 * (fm_index["suffix_array"]: n+1 entries, 1-based starts, row 0 = n+1; SMEM/ExactMatch.py:66).
 * Used by ExactMatch.load_fm_index on files the reference wrote. */
int genie_index_create_from_sa(const uint8_t *codes, int64_t n, const int32_t *sa_one_based, int32_t K,
                               int32_t dir_bits, genie_index **out);

/* genie_index_create / _from_sa (sa_one_based may be NULL) with the size of the per-P2-mer tables chosen by
 * the caller: table_bits = P2 in (dir_bits, 12] (anything else but 0 is GENIE_E_INVALID), 0 = automatic (smallest P2 with 4^P2 >= n/4: measured best on MI355X at n = 100 kb and 1 Mb).  A tuning
 * knob of the index image only: results do not depend on it.  The form of the per-P2-mer match table is chosen the same
 * way: GENIE_TABLE_WIDE / GENIE_TABLE_COMPACT ORed into table_bits, neither = automatic (compact: 16-byte entries, for
 * every reference of fewer than 2^24 bases). */
#define GENIE_TABLE_WIDE (1 << 8)    /* OR into table_bits: 32-byte entries with 16-base keys */
#define GENIE_TABLE_COMPACT (2 << 8) /* OR into table_bits: 16-byte entries with 8-base keys (n < 2^24) */
int genie_index_create_ex(const uint8_t *codes, int64_t n, const int32_t *sa_one_based, int32_t K, int32_t dir_bits,
                          int32_t table_bits, genie_index **out);

/* Install an RMI model (RMI.models after RMI.fit, SMEM/RMI.py:10-50): `nlev` levels, level l has
 * sizes[l] linear models (sizes[0] == 1) and the clamp scale scales[l] (= experts + [1], RMI.py:54);
 * coef / icpt are the per-level arrays concatenated.  Must precede serialize / to_device. */
int genie_index_set_rmi(genie_index *ix, int32_t nlev, const int32_t *sizes, const int32_t *scales,
                        const double *coef, const double *icpt);

/* Train the RMI natively (no scikit-learn): RMI_LUT.train_RMI + RMI.fit (SMEM/RMI_LUT.py:36-50,
 * SMEM/RMI.py:10-50) on the handle's own (K-mer code, SA row) pairs, `experts` as in
 * RMI_LUT(structure=experts, ...), e.g. {1000} or {10, 100}; closed-form least squares per expert with
 * the reference's bucket-budget targets.  Installs the model like genie_index_set_rmi and also records a
 * per-leaf error bound (max |int(prediction) - row| over the training pairs) that the device uses to
 * fence the last-mile search of genie_seed_lookup.  Outputs (optional): mean and max of that error.
 * Coefficients differ from scikit-learn's in the last bits, which only moves where a search starts. */
int genie_index_train_rmi(genie_index *ix, int32_t n_experts, const int32_t *experts, double *mean_abs_err,
                          int32_t *max_abs_err);
/* Export the installed model: coef / icpt hold all levels concatenated (1 + experts[0] + ... entries);
 * leaf_err (optional, natively trained models only) one bound per model of the last level. */
int genie_index_rmi_models(const genie_index *ix, double *coef, double *icpt, int32_t *leaf_err);

int genie_index_info(const genie_index *ix, genie_info *out);

/* Host views for the position-resolution helpers of the drop-in API
 * (ExactMatch.get_position(s) / exact_match, SMEM/ExactMatch.py:174-199).
 * 1-based values as the reference stores them; NULL when the handle has no host arrays. */
const int32_t *genie_index_suffix_array(const genie_index *ix);
/* Sorted distinct K-mer table (the reference's lut dict in key order): codes/lo/hi[lut_keys]. */
int genie_index_lut_arrays(const genie_index *ix, const uint32_t **codes, const int32_t **lo, const int32_t **hi);

/* Serialize to one flat, position-independent image (header + sections).  The caller uploads
 * it (e.g. torch.from_numpy(buf).cuda()) and -- multi-GPU -- broadcasts that ONE tensor over
 * RCCL; every rank then calls genie_index_open on its copy. */
int64_t genie_index_blob_bytes(const genie_index *ix);
int genie_index_serialize(const genie_index *ix, void *host_dst, int64_t cap);

/* The same with options.  GENIE_IMAGE_NO_SEED_TABLE leaves out the K-mer hash table (half of the image at 1 Mb): for ranks
 * that only run genie_find_smems* / genie_sa_interval / genie_locate -- genie_seed_lookup(LUT) on such an image returns
 * GENIE_E_NO_LUT.  (What a multi-GPU driver broadcasts.) */
#define GENIE_IMAGE_NO_SEED_TABLE 1
int64_t genie_index_image_bytes(const genie_index *ix, int32_t image_flags);
int genie_index_serialize_image(const genie_index *ix, int32_t image_flags, void *host_dst, int64_t cap);

/* Open a device-resident image.  `host_header` = the first GENIE_HEADER_BYTES of the same
 * image in host memory (ranks that received it by broadcast copy those bytes back).  The
 * image is NOT copied and must outlive the handle.  If `ix_inout` points at an existing handle
 * the image is bound to it (keeps the host arrays); otherwise a device-only handle is made. */
int genie_index_open(const void *host_header, const void *d_blob, int64_t blob_bytes, int32_t device,
                     genie_index **ix_inout);

/* Check the CONTENTS of an opened image on the device (genie_index_open checks the header only): every row number,
 * entry index and suffix start that a kernel will later follow must lie inside its section.  One pass over the image on
 * `stream`, then a synchronisation.  GENIE_E_BAD_BLOB when something is out of range (*what, optional, gets a bit per
 * section: 1 suffix array, 2 prefix directory, 4 range table, 8 / 16 match table / its overflow links, 32 K-mer table,
 * 64 RMI error bounds).  The drop-in calls it on every image it opens, also on one received by broadcast. */
int genie_index_validate(const genie_index *ix, uint32_t *what, void *stream);

/* ---------------------------------------------------------------------------------------
 * Index construction on the device: genie_index_create_ex + genie_index_serialize_image + genie_index_open in one call,
 * for a reference that is already in device memory.  The image bytes are the ones the host path writes (the host builder
 * stays the specification; the tests compare the two byte for byte).
 *   d_codes     n base codes (0..3) in device memory;
 *   K, dir_bits, table_bits   as genie_index_create_ex (table_bits may carry GENIE_TABLE_WIDE / GENIE_TABLE_COMPACT);
 *   image_flags GENIE_IMAGE_NO_SEED_TABLE or 0, as genie_index_serialize_image;
 *   d_image     caller-owned, 256-byte aligned, image_cap >= genie_index_device_image_bound(...) bytes; *image_bytes gets
 *               the size of the image written at its front (the rest of the buffer is unused);
 *   d_tmp       caller-owned, 256-byte aligned scratch of genie_index_device_build_tmp_bytes(...) bytes: about 14 four-byte
 *               words per base (suffix-array sort buffers, neighbour LCPs, the K-mer list and hash-table placement) plus
 *               about 4.2 words per P2-mer (per-prefix row tables);
 *   device, stream  the HIP device (made current) and stream of every launch; the call synchronizes `stream` once, at the
 *               end (the header has to reach the host).
 * Errors as genie_index_create_ex: GENIE_E_ALPHABET for a code > 3 (found on the device, reported after the build),
 * GENIE_E_INVALID for n, K, table_bits or image_flags out of range, a null or misaligned pointer, or image_cap / tmp_bytes
 * too small -- all checked before any device work.
 * The returned handle is device-only, like one from genie_index_open on a received image: no host arrays
 * (genie_index_suffix_array / genie_index_lut_arrays give NULL / GENIE_E_INVALID, genie_index_serialize* GENIE_E_INVALID),
 * no RMI model (GENIE_MODE_RMI gives GENIE_E_NO_MODEL; genie_index_set_rmi / genie_index_train_rmi refuse it with
 * GENIE_E_INVALID).  The image must outlive the handle; it can be broadcast and opened elsewhere like any other.
 * The bound and scratch functions return GENIE_E_INVALID (negative) for arguments create_device would refuse. */
int64_t genie_index_device_image_bound(int64_t n, int32_t K, int32_t dir_bits, int32_t table_bits);
int64_t genie_index_device_build_tmp_bytes(int64_t n, int32_t K, int32_t dir_bits, int32_t table_bits);
int genie_index_create_device(const uint8_t *d_codes, int64_t n, int32_t K, int32_t dir_bits, int32_t table_bits,
                              int32_t image_flags, void *d_image, int64_t image_cap, int64_t *image_bytes, void *d_tmp,
                              int64_t tmp_bytes, int32_t device, void *stream, genie_index **out);

/* Convenience for non-torch callers: hipMalloc + upload an image owned by the handle. */
int genie_index_to_device(genie_index *ix, int32_t device);

void genie_index_destroy(genie_index *ix);

/* ---------------------------------------------------------------------------------------
 * Hot path (device).  All launches are asynchronous on `stream`.
 * ------------------------------------------------------------------------------------- */

/* Batched ExactMatch.exact_match_back_prop (SMEM/ExactMatch.py:132-151):
 * pattern i = d_pats[i*stride .. +len_i) with len_i = d_lens ? d_lens[i] : fixed_len;
 * d_out_lohi[2i..2i+1] = inclusive SA interval, or (-1,-1) if absent; an empty pattern gives
 * (0, n) like the reference; a code > 3 gives (-2,-2) (reference: KeyError). */
int genie_sa_interval(const genie_index *ix, const uint8_t *d_pats, const int32_t *d_lens, int64_t N,
                      int32_t stride, int32_t fixed_len, int32_t *d_out_lohi, void *stream);

/* Batched seed lookup of one K-mer each (N rows of K codes, row stride K):
 * mode LUT: `lut[str(code)][0]` membership + interval (SMEM/SMEM.py:28-32,65-67);
 * mode RMI: RMI_LUT.get_suffix_rmi = predict + last-mile search (SMEM/RMI_LUT.py:67-184),
 * contract behaviour = the true interval; an absent K-mer is reported the reference's way,
 * lower > upper (lower = the row it would be inserted at).  LUT output as genie_sa_interval.
 * A reference of fewer than K bases holds no K-mer: every K-mer is absent, in each mode's own way
 * (genie_index_train_rmi refuses such a handle with GENIE_E_INVALID; genie_index_set_rmi does not).
 * d_pred (may be NULL,
 * RMI only) receives the float64 prediction of RMI_LUT.rmi_predict (SMEM/RMI_LUT.py:53-63). */
int genie_seed_lookup(const genie_index *ix, int32_t mode, const uint8_t *d_kmers, int64_t N,
                      int32_t *d_out_lohi, double *d_pred, void *stream);

/* Batched SMEM discovery: replaces SMEM.get_SMEMS / get_smems_lut / get_smems_rmi.
 * Read r = d_reads[r*stride .. +len_r), len_r = d_lens ? d_lens[r] : fixed_len.
 * Writes d_counts[r] = number of SMEMs of read r (after the min_len filter, which the
 * reference applies in BWA mode only, SMEM.py:463; pass 1 otherwise) and
 * d_slots[(r*cap + t)*4 + {0,1,2,3}] = (start, end, lo, hi) of its t-th SMEM in the
 * reference's emission order: the substring read[start:end) and its SA interval [lo, hi].
 * d_status[r] (may be NULL) = GENIE_READ_* code.  `cap` slots per read (cap >= max read
 * length never overflows).
 * d_workspace: 256-byte aligned device scratch of genie_find_smems_workspace_bytes(N, max_len)
 * bytes (matching statistics, packed reads and emitted (start, end) pairs handed between
 * the kernels of the pipeline). */
int64_t genie_find_smems_workspace_bytes(int64_t N, int32_t max_len);
/* Per-read rows of that workspace, for traffic accounting: out[0] = bytes of a matching-statistics (fwd) row,
 * out[1] = 16-byte pieces of the packed read (reads of up to 255 bases: plain 64-bit words, two per piece; longer: overlapping
 * records {w[i], w[i+1]}), out[2] = 0 (reserved), out[3] = bytes of the emitted
 * (count, (start, end) pairs) row. */
int genie_find_smems_workspace_rows(int32_t max_len, int32_t *row_bytes4);
int genie_find_smems(const genie_index *ix, int32_t mode, const uint8_t *d_reads, const int32_t *d_lens,
                     int64_t N, int32_t stride, int32_t fixed_len, int32_t min_len, int32_t *d_counts,
                     int32_t *d_slots, int32_t cap, int32_t *d_status, void *d_workspace, int64_t workspace_bytes,
                     void *stream);

/* Same discovery, CSR output in one call: d_offsets[N+1] = exclusive prefix sum of the per-read SMEM
 * counts, d_rows[4*t .. 4*t+3] = (start, end, lo, hi) of SMEM t, reads in input order, SMEMs in the
 * reference's emission order.  Every row is written exactly once; rows beyond out_cap_rows are
 * dropped (the caller compares d_offsets[N] with its capacity).  Flagged reads contribute no rows. */
int genie_find_smems_csr(const genie_index *ix, int32_t mode, const uint8_t *d_reads, const int32_t *d_lens,
                         int64_t N, int32_t stride, int32_t fixed_len, int32_t min_len, int64_t *d_offsets,
                         int32_t *d_rows, int64_t out_cap_rows, int32_t *d_status, void *d_workspace,
                         int64_t workspace_bytes, void *stream);

/* SMEMs of both strands of every read in one call.  Inputs as genie_find_smems_csr: uint8 [N, stride] codes, d_lens (may
 * be NULL: fixed_len for every read; with d_lens, fixed_len is the longest length), reads of at most GENIE_MAX_READ_LEN
 * bases, every mode, min_len applied in BWA mode.  The output covers 2N strand-reads, interleaved: strand-read 2i + s is
 * read i when s = 0 and its reverse complement rc(read i) when s = 1 (reversed, code c -> 3 - c).
 *   d_offsets[2N+1]  offsets of the CSR rows;  d_rows  int32 rows (start, end, lo, hi), 16-byte aligned;
 *   d_status[2N]     one GENIE_READ_* code per strand-read (may be NULL): a reference without T gives
 *                    GENIE_READ_ABSENT_BASE on the reverse strand of a read that holds an A and GENIE_READ_OK on its forward one;
 *   rows past out_cap_rows are dropped, d_offsets[2N] still holds the true total.
 * Defining property: the output is byte for byte what genie_find_smems_csr returns for the batch
 * [r0, rc(r0), r1, rc(r1), ...] with each length given twice.  The reverse complement is never written to memory: the
 * match-statistics kernel builds it while packing the read.
 * On strand 1, start / end are positions in the reverse-complemented read (the rows SMEM.get_SMEMS(rc(q), m) /
 * get_smems_lut / get_smems_rmi give); in forward coordinates of a read of length L the SMEM covers
 * [L - end, L - start).  The rows are left as they are.  The two strands' sets are computed independently: a
 * reverse-strand SMEM contained in a forward one is not removed (as with two calls).
 * d_workspace: 256-byte aligned, genie_find_smems_both_workspace_bytes(N, max_len) bytes with max_len >= fixed_len
 * (at least genie_find_smems_workspace_bytes(2N, max_len)).  Argument checks come before the device check, so they hold on
 * any handle: bad pointers or sizes (stride < fixed_len included) give GENIE_E_INVALID, fixed_len > GENIE_MAX_READ_LEN
 * GENIE_E_TOO_LONG, a small or misaligned workspace GENIE_E_CAPACITY.  N = 0 writes d_offsets[0] = 0.  No stream
 * synchronization.  The workspace size function returns GENIE_E_INVALID for negative arguments and GENIE_E_TOO_LONG
 * above GENIE_MAX_READ_LEN. */
int64_t genie_find_smems_both_workspace_bytes(int64_t N, int32_t max_len);
int genie_find_smems_both(const genie_index *ix, int32_t mode, const uint8_t *d_reads, const int32_t *d_lens, int64_t N,
                          int32_t stride, int32_t fixed_len, int32_t min_len, int64_t *d_offsets, int32_t *d_rows,
                          int64_t out_cap_rows, int32_t *d_status, void *d_workspace, int64_t workspace_bytes, void *stream);

/* SMEMs of reads that contain breaks (ambiguous bases such as N), where genie_find_smems* flag the whole read instead.
 * A break is a position whose code is > 3 (any byte 4..255) or whose base never occurs in the reference; a segment is a
 * maximal run of positions that are not breaks.  No exact match covers a break, so the SMEMs of a read are the union of
 * its segments' SMEMs: segments in read order, each with SMEM.get_SMEMS's emission order and min_len filter (the BWA
 * traversal; a segment shorter than K is searched like any other), start / end positions in the whole read, lo / hi
 * unchanged.  Inputs and outputs as genie_find_smems_csr (there is no mode argument): d_offsets[N+1], int32 rows
 * (start, end, lo, hi), rows beyond out_cap_rows dropped with d_offsets[N] still the true total.  d_lens may be NULL;
 * with d_lens, fixed_len is the longest length and every d_lens[r] must lie in [0, fixed_len] (GENIE_E_INVALID,
 * found on the device, otherwise).  d_status[r] (may be NULL) = GENIE_READ_OK: a read of length 0 or made only of
 * breaks has no rows.
 * d_workspace: 256-byte aligned, genie_find_smems_split_workspace_bytes(N, max_len) bytes with max_len >= fixed_len
 * (GENIE_E_CAPACITY when smaller).  Argument checks come before the device check, so they hold on any handle.
 * Unlike the other hot-path calls this one synchronizes `stream`: once to learn whether any read has a break or is
 * empty (when none has, the reads go through the genie_find_smems_csr pipeline unchanged, byte for byte the same output);
 * otherwise once more for the segment totals, and once per extra pass when the segments outnumber what the workspace
 * holds (passes of at least N segments). */
int64_t genie_find_smems_split_workspace_bytes(int64_t N, int32_t max_len);
int genie_find_smems_split(const genie_index *ix, const uint8_t *d_reads, const int32_t *d_lens, int64_t N, int32_t stride,
                           int32_t fixed_len, int32_t min_len, int64_t *d_offsets, int32_t *d_rows, int64_t out_cap_rows,
                           int32_t *d_status, void *d_workspace, int64_t workspace_bytes, void *stream);

/* SMEMs of reads of ANY length (genie_find_smems_csr is limited to GENIE_MAX_READ_LEN bases).  The reads come as CSR:
 * read r is d_bases[d_read_offsets[r] .. d_read_offsets[r+1]) (codes 0..3; N+1 offsets, int64, on the device), any length
 * from 0 to 2^31 - 1.  total_bases and max_len are host-side bounds: every offset must lie in [0, total_bases] and no read
 * may be longer than max_len; offsets that decrease or break a bound give GENIE_E_INVALID (checked on the device).
 * Output as genie_find_smems_csr: d_offsets[N+1], int32 rows (start, end, lo, hi) in input order and get_SMEMS order,
 * min_len applied in BWA mode, rows past out_cap_rows dropped (d_offsets[N] still the true total), d_status[r] (may be
 * NULL) the same GENIE_READ_* codes.  For every read that genie_find_smems_csr accepts, rows and status are the same bytes.
 * d_rows 16-byte aligned; d_workspace 256-byte aligned, genie_find_smems_long_workspace_bytes(N, total_bases, max_len)
 * bytes (GENIE_E_CAPACITY when smaller): about 17.3 bytes per base plus 48 per read.  Argument checks come before the
 * device check.  This call synchronizes `stream` once, after the offset check and before any other kernel runs.
 * Both functions are genie_find_smems_long_ex (below) with flags == 0: the same checks, workspace and launches.
 * Batch sizes, for this call and for genie_find_smems_long_ex, genie_match_stats, genie_exact_match, genie_reads_from_text,
 * genie_reads_from_fasta and genie_locate: N, total_bases, text_bytes, out_cap_rows, cap_positions and every offset are
 * 64-bit and are used as such; 2^24 reads, units or windows, 2^31 bases or bytes and 2^32 virtual positions are ordinary
 * (kernels with one block per 256-position window are launched in slices once a launch would pass HIP's 2^32 threads).
 * What a single launch still cannot cover returns GENIE_E_TOO_LONG (the outputs are then undefined): 2^32 or more strand-reads,
 * strand-patterns, units of one pass, intervals or windows (total_bases / 256 + units + 1); 2^32 words of the packed stream
 * (total_bases / 32 + 3 units + 4); 2^38 virtual positions with GENIE_READS_SPLIT_BREAKS; a text of 2^36 bytes, or one of
 * 2^32 bytes with cap_reads as large.  The smallest of these (2^32 intervals for genie_locate) takes some 80 GB of caller
 * buffers. */
int64_t genie_find_smems_long_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len);
int genie_find_smems_long(const genie_index *ix, int32_t mode, const uint8_t *d_bases, const int64_t *d_read_offsets,
                          int64_t N, int64_t total_bases, int64_t max_len, int32_t min_len,
                          int64_t *d_offsets, int32_t *d_rows, int64_t out_cap_rows, int32_t *d_status,
                          void *d_workspace, int64_t workspace_bytes, void *stream);

/* genie_find_smems_long with both strands and / or breaks.  Inputs as genie_find_smems_long (CSR reads of any length,
 * total_bases / max_len as host-side bounds, the same offset check on the device); `flags` ORs
 *   GENIE_READS_BOTH_STRANDS  the output covers 2N strand-reads, interleaved as genie_find_smems_both: strand-read 2i is
 *                             read i, 2i + 1 is rc(read i) (reversed, code c -> 3 - c, a code > 3 stays what it is);
 *                             d_offsets[2N+1], d_status[2N]; strand-1 rows keep positions in the reverse complement;
 *   GENIE_READS_SPLIT_BREAKS  the semantics of genie_find_smems_split: a break is a position whose code is > 3 or whose
 *                             base (on a reversed strand: its complement) never occurs in the reference; a strand-read's
 *                             SMEMs are those of its segments, in its own order, each with the BWA traversal and min_len,
 *                             start / end in the whole strand-read; every status GENIE_READ_OK; an empty or all-break
 *                             strand-read has no rows.  Only with GENIE_MODE_BWA (GENIE_E_INVALID otherwise).
 * Let S = 2 with BOTH_STRANDS, else 1.  Defining properties, each byte for byte:
 *   flags == 0         what genie_find_smems_long documents: that call is this one with no flags, and so is its
 *                      workspace function;
 *   BOTH_STRANDS       genie_find_smems_long on the explicit batch [r0, rc(r0), r1, rc(r1), ...], every mode, status per
 *                      strand-read -- and so genie_find_smems_both on reads of at most GENIE_MAX_READ_LEN bases;
 *   SPLIT_BREAKS       genie_find_smems_split on reads of at most GENIE_MAX_READ_LEN bases;
 *   both               SPLIT_BREAKS alone on that explicit interleaved batch.
 * Rows past out_cap_rows are dropped and d_offsets[S N] keeps the true total; N = 0 writes d_offsets[0] = 0.  Unknown flag
 * bits, bad pointers / sizes / alignment give GENIE_E_INVALID and a small workspace GENIE_E_CAPACITY, all before the device
 * check; bad offsets GENIE_E_INVALID, found on the device.  The reverse complement is never written to memory as bytes.
 * d_workspace: 256-byte aligned, genie_find_smems_long_ex_workspace_bytes(N, total_bases, max_len, flags) bytes: the
 * long-read pipeline for S total_bases positions and S N units (one at least with any flag; a unit is one strand of one
 * segment of one read), i.e. about 17.3 S bytes per base and 64 S per read; with SPLIT_BREAKS one more unit per 32
 * positions, the unit table and the segmentation's counts: about 20.1 S bytes per base and 92 S per read.
 * Synchronisations of `stream`: without SPLIT_BREAKS one, after the offset check (as genie_find_smems_long).  With it one
 * more to read the number of units, and one per extra pass when the units outnumber what the workspace holds (passes of
 * consecutive units, each of at least S N). */
#define GENIE_READS_BOTH_STRANDS 1
#define GENIE_READS_SPLIT_BREAKS 2
int64_t genie_find_smems_long_ex_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags);
int genie_find_smems_long_ex(const genie_index *ix, int32_t mode, int32_t flags, const uint8_t *d_bases,
                             const int64_t *d_read_offsets, int64_t N, int64_t total_bases, int64_t max_len,
                             int32_t min_len, int64_t *d_offsets, int32_t *d_rows, int64_t out_cap_rows,
                             int32_t *d_status, void *d_workspace, int64_t workspace_bytes, void *stream);

/* Matching statistics of EVERY position of every read: how far the longest match that starts there reaches, and its
 * suffix-array interval -- the batched form of SMEM.forward_extension (SMEM.py:425-443), and the quantity every SMEM
 * call derives its rows from.  Inputs as genie_find_smems_long_ex (CSR reads of any length, total_bases / max_len as
 * host-side bounds, the same offset check on the device); `flags` ORs GENIE_READS_BOTH_STRANDS and
 * GENIE_READS_SPLIT_BREAKS with the meanings they have there; S = 2 with BOTH_STRANDS, else 1.  There is no mode: the BWA
 * traversal's input checks apply, so no read is GENIE_READ_TOO_SHORT.
 * Layout: the virtual positions of the strand-reads back to back.  Position p of strand-read S i + s (read i of L_i bases
 * at d_read_offsets[i] = o_i, strand s) is element v = S o_i + s L_i + p: on one strand d_ms lies parallel to d_bases.
 * Strand 1 is the reverse complement and p a position in it, as for rows.
 *   d_ms[v]    (S total_bases int32) the largest l >= 0 such that the l bases of the strand-read from p on hold no break
 *              and occur in the reference.  A break is a code > 3; with SPLIT_BREAKS also a base the reference lacks
 *              (without it such a base has l = 0 all the same: it occurs nowhere).
 *   d_lohi[2v], d_lohi[2v + 1]  (2 S total_bases int32, may be NULL: lengths only) the inclusive suffix-array interval of
 *              that match, what genie_sa_interval returns for it; (-1, -1) where l == 0.
 *   d_status[S i + s]  (S N int32, may be NULL) without SPLIT_BREAKS: GENIE_READ_BAD_BASE for a strand-read that holds a code
 *              > 3 -- all its d_ms are then -1 and all its d_lohi (-1, -1) --, GENIE_READ_ABSENT_BASE for one that holds a
 *              base the reference lacks, whose values are written and correct all the same; else GENIE_READ_OK.  With
 *              SPLIT_BREAKS every status is GENIE_READ_OK.
 * After the call every element of the three arrays is defined: break positions hold 0 and (-1, -1), and so do the
 * elements in front of S d_read_offsets[0] and from S d_read_offsets[N] on, which belong to no read.  Nothing outside the
 * declared sizes is written.  N = 0 and total_bases = 0 are fine.  ms[v + 1] >= ms[v] - 1 inside a strand-read.
 * Defining property, byte for byte: with BOTH_STRANDS the three outputs are those of the call without it on the explicit
 * batch [r0, rc(r0), r1, rc(r1), ...].
 * Checked before the device check, so on any handle: a null ix, d_read_offsets (N > 0), d_bases or d_ms (total_bases >
 * 0), a negative size, max_len above 2^31 - 1, an unknown flag bit, d_ms not 4-byte or d_lohi not 8-byte aligned give
 * GENIE_E_INVALID; then, for N > 0, a d_workspace that is null, not 256-byte aligned or smaller than
 * genie_match_stats_workspace_bytes(N, total_bases, max_len, flags) gives GENIE_E_CAPACITY.  Bad offsets give
 * GENIE_E_INVALID, found on the device.  The workspace function returns GENIE_E_INVALID for arguments the call would
 * refuse; it never exceeds genie_find_smems_long_ex_workspace_bytes of the same arguments (two of that pipeline's five
 * stages run: about 4.3 S bytes per base and 28 per read, 44 S with both strands; with SPLIT_BREAKS 6.1 S and 64 S).
 * Synchronisations of `stream`: one, after the offset check; with SPLIT_BREAKS one more to read the number of units.
 * Extra unit passes (units outnumbering what the workspace holds) cost none: no row count has to reach the host.
 * Cost: the interval of a match of l bases that lies inside a repeat of the reference takes a suffix-array search whose
 * probes compare up to l bases each; a read that follows a tandem repeat pays that at every one of its positions. */
int64_t genie_match_stats_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags);
int genie_match_stats(const genie_index *ix, int32_t flags, const uint8_t *d_bases, const int64_t *d_read_offsets,
                      int64_t N, int64_t total_bases, int64_t max_len,
                      int32_t *d_ms,        /* S * total_bases */
                      int32_t *d_lohi,      /* 2 * S * total_bases, may be NULL */
                      int32_t *d_status,    /* S * N, may be NULL */
                      void *d_workspace, int64_t workspace_bytes, void *stream);

/* The suffix-array interval of every pattern of a batch given as CSR, on one strand or both: the batched form of
 * ExactMatch.exact_match_back_prop (ExactMatch.py:132-151) for patterns of ANY length.  genie_sa_interval takes a padded
 * matrix of patterns of at most GENIE_MAX_READ_LEN bases and gives each pattern a whole wave; here every pattern has its own
 * length and one lane, and a batch of mixed lengths costs its bases, not N times its longest pattern.
 * Inputs: pattern i is d_bases[d_pat_offsets[i] .. d_pat_offsets[i+1]) (codes 0..3; N+1 offsets, int64, on the device), any
 * length from 0 to 2^31 - 1.  total_bases and max_len are host-side bounds, as for genie_find_smems_long: every offset must
 * lie in [0, total_bases] and no pattern may be longer than max_len (checked on the device).  The offsets need not begin at 0
 * nor end at total_bases: the bytes of d_bases outside [d_pat_offsets[0], d_pat_offsets[N]) are ignored.
 * `flags`: GENIE_READS_BOTH_STRANDS or 0.  Any other bit gives GENIE_E_INVALID, GENIE_READS_SPLIT_BREAKS included (a pattern
 * with a break has no interval).  S = 2 with the flag, else 1.  Strand-pattern q = S i + s is pattern i for s = 0 and its
 * reverse complement for s = 1 (reversed, code c -> 3 - c, a code > 3 stays what it is), interleaved as
 * genie_find_smems_both's strand-reads.  The reverse complement is never written to memory as bytes.
 * Outputs, for strand-pattern q:
 *   d_lohi[2q], d_lohi[2q + 1]  (2 S N int32) what genie_sa_interval gives for that pattern: the inclusive interval of the
 *              suffix-array rows whose suffix starts with it; (-1, -1) if it occurs nowhere -- a base that the reference
 *              lacks is nothing special, the pattern is simply absent --; (0, n) for the empty pattern; (-2, -2) if it
 *              holds a code > 3.
 *   d_counts[q]  (S N int32, may be NULL) its occurrences, hi - lo + 1: 0 where absent or bad, n + 1 for the empty pattern.
 *   d_status[q]  (S N int32, may be NULL) GENIE_READ_BAD_BASE for (-2, -2), else GENIE_READ_OK.
 * After the call every element of the three arrays is defined and nothing outside the declared sizes is written.  N = 0
 * writes nothing and returns GENIE_OK; total_bases = 0 with N > 0 is a batch of empty patterns.  The output is a function of
 * the inputs alone (no atomic decides a value).
 * Defining properties, each byte for byte:
 *   flags == 0     on patterns of at most GENIE_MAX_READ_LEN bases d_lohi is what genie_sa_interval writes for the same
 *                  patterns padded into a matrix;
 *   BOTH_STRANDS   the three outputs are those of the call without the flag on the explicit batch
 *                  [p0, rc(p0), p1, rc(p1), ...].
 * Checked before the device check, so on any handle: a null ix, a null d_pat_offsets or d_lohi (N > 0), a null d_bases
 * (total_bases > 0), a negative size, max_len above 2^31 - 1, a flag bit other than BOTH_STRANDS, d_lohi not 8-byte or
 * d_counts / d_status not 4-byte aligned give GENIE_E_INVALID; then, for N > 0, a d_workspace that is null, not 256-byte
 * aligned or smaller than genie_exact_match_workspace_bytes(N, total_bases, max_len, flags) gives GENIE_E_CAPACITY.  Offsets
 * that decrease or break a bound give GENIE_E_INVALID, found on the device; the outputs are then not written.
 * The workspace function returns GENIE_E_INVALID for arguments the call would refuse, is monotone in N and total_bases and
 * a multiple of 256, does not depend on max_len, and never exceeds genie_match_stats_workspace_bytes of the same arguments
 * (one of that pipeline's stages runs, the packed stream: 0.25 S bytes per base -- 8 per 32 bases -- and 28 per pattern,
 * 88 with both strands: a status word and three padding words per strand-pattern, and 16 for its entry of the strand table).
 * Synchronisations of `stream`: one, after the offset check and before any other kernel runs.  No others.
 * Cost: when max_len is at most 64 every lane packs its own pattern from d_bases; above that the whole batch first goes
 * through the long-read pack stage, which then takes most of the call's time, so give max_len tightly and keep batches of
 * short patterns apart from long ones.  A pattern of at most dir_bits bases is two directory reads; a longer one is a search of its bucket whose probes
 * compare up to its length when it lies inside a repeat of the reference.  Lanes of a wave work on unrelated patterns, so
 * a wave takes as long as its slowest pattern: sort a batch by length if its lengths differ by orders of magnitude. */
int64_t genie_exact_match_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags);
int genie_exact_match(const genie_index *ix, int32_t flags, const uint8_t *d_bases, const int64_t *d_pat_offsets,
                      int64_t N, int64_t total_bases, int64_t max_len,
                      int32_t *d_lohi,      /* 2 * S * N */
                      int32_t *d_counts,    /* S * N, may be NULL */
                      int32_t *d_status,    /* S * N, may be NULL */
                      void *d_workspace, int64_t workspace_bytes, void *stream);

/* Every maximal exact match (MEM) of at least min_len bases of every strand-read, with its reference position: MUMmer's
 * -maxmatch, the input of chaining and dot-plots.  The SMEM calls report only matches that no other match of the read
 * contains, and genie_match_stats only the longest match from each position; this call reports every occurrence.
 * Inputs and flags are those of genie_match_stats: CSR reads of any length, total_bases / max_len as host-side bounds, the
 * same offset check on the device, GENIE_READS_BOTH_STRANDS and GENIE_READS_SPLIT_BREAKS with the same meanings; S = 2 with
 * BOTH_STRANDS, else 1; on strand 1 positions are in the reverse complement.
 * Definition.  The reference T has n bases, a strand-read Q has L, m = min_len >= 1.  A break is a position of Q whose
 * code is > 3, with SPLIT_BREAKS also one whose base the reference lacks; a break equals nothing.  A MEM is (p, t, l)
 * with l >= m, Q[p .. p+l) == T[t .. t+l) base for base, no break inside, and
 *   right-maximal   p + l == L, or t + l == n, or Q[p+l] != T[t+l];
 *   left-maximal    p == 0, or t == 0, or Q[p-1] != T[t-1].
 * Output: d_offsets[S N + 1] and int32 rows (start, end, pos, row) = (p, p + l, t + 1, r): pos is 1-based, what
 * genie_locate returns, and r is the suffix-array row of suffix t.  The rows of a strand-read are ordered by (start
 * ascending, row ascending), strand-reads are in input order: the output is a function of the inputs alone (no atomic
 * decides a value).  Rows past out_cap_rows are dropped and d_offsets[S N] keeps the true total; d_rows == NULL is the
 * sizing call (offsets and totals are written all the same); N = 0 writes d_offsets[0] = 0.
 *   d_status[S i + s]  (S N int32, may be NULL) what genie_match_stats writes.  Without SPLIT_BREAKS a strand-read flagged
 *              GENIE_READ_BAD_BASE has no rows; one flagged GENIE_READ_ABSENT_BASE keeps its rows.
 *   d_totals   (2 int64, may be NULL) {rows in all, positions skipped by max_occ}.
 *   max_occ    0: no limit.  max_occ > 0: a position whose seed Q[p .. p+m) has more than max_occ occurrences in the
 *              reference contributes no rows and is counted in d_totals[1].  This bounds the work; it is no seeding policy.
 * Two consequences: the rows that start at p and are ms[p] long are the rows of genie_match_stats's lohi[p] whose occurrence
 * is left-maximal; and every row (s, e, lo, hi) of genie_find_smems_long_ex (same flags, BWA mode) with e - s >= m gives a
 * row (s, e, SA[r] + 1, r) of this call for every r in [lo, hi].
 * Checked before the device check, so on any handle: a null ix, d_offsets or d_read_offsets, a null d_bases (total_bases >
 * 0), a negative size, min_len < 1, max_occ < 0, max_len above 2^31 - 1, an unknown flag bit, d_rows not 16-byte, d_offsets
 * or d_totals not 8-byte or d_status not 4-byte aligned give GENIE_E_INVALID; then, for N > 0, a d_workspace that is null,
 * not 256-byte aligned or smaller than genie_find_mems_workspace_bytes(N, total_bases, max_len, flags) gives
 * GENIE_E_CAPACITY.  Bad offsets give GENIE_E_INVALID, found on the device; GENIE_E_TOO_LONG on the single-launch limits of
 * genie_match_stats.  The workspace function returns GENIE_E_INVALID for arguments the call would refuse, is a multiple of
 * 256, monotone in N and total_bases, does not depend on max_len and is at least genie_match_stats_workspace_bytes of the
 * same arguments: that workspace plus 33 S bytes per base (ms 4, lohi 8, the seed's rows 8, the position in its strand-read
 * 4, the base in front 1, the row offset inside its block 8) and 8 per 64 positions, i.e. about 37.4 S bytes per base and
 * 28 per read (44 S with both strands; with SPLIT_BREAKS 39.2 S and 64 S).
 * Synchronisations of `stream`: those of genie_match_stats and no more; the row total stays on the device.
 * Cost: genie_match_stats with intervals, then per position with ms >= m the rows of its seed -- two directory reads when m
 * is at most dir_bits, else two bisections of the seed's directory bucket (one 16-byte row per probe, the packed reference
 * only past dir_bits + 32 bases) --, then twice (count, fill) one suffix-array row and one reference base for EVERY
 * occurrence of the seed, left-maximal or not: on a repeat-rich reference with a small min_len the call's time is the
 * number of seed occurrences, which max_occ bounds.  A row outside the longest match's interval costs a word-wise
 * comparison of two reference suffixes up to its length. */
int64_t genie_find_mems_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags);
int genie_find_mems(const genie_index *ix, int32_t flags, const uint8_t *d_bases, const int64_t *d_read_offsets,
                    int64_t N, int64_t total_bases, int64_t max_len, int32_t min_len, int32_t max_occ,
                    int64_t *d_offsets,      /* S * N + 1 */
                    int32_t *d_rows,         /* 4 * out_cap_rows, 16-byte aligned; may be NULL: counting only */
                    int64_t out_cap_rows,
                    int32_t *d_status,       /* S * N, may be NULL */
                    int64_t *d_totals,       /* 2, may be NULL: {rows in all, positions skipped by max_occ} */
                    void *d_workspace, int64_t workspace_bytes, void *stream);

/* A reference of SEVERAL sequences (chromosomes, scaffolds, plasmids): one index over their concatenation plus a contig
 * table.  Without the table every call answers in the concatenation's coordinates and reports, without a word, matches that
 * start in one sequence and end in the next; such a match exists in no molecule.
 * Definitions.  A contig table is d_contig_offsets: a device array of n_contigs + 1 int64 values, n_contigs >= 1, 8-byte
 * aligned, with off[0] = 0, non-decreasing values and off[n_contigs] = n, the reference length of the handle.  Contig c
 * is T[off[c] .. off[c+1]); it may be empty (FASTA records may be).  The contig of a 0-based reference position t < n is the
 * unique c with off[c] <= t < off[c+1] (empty contigs own nothing); room(t) = off[c+1] - t; t is a contig start iff t ==
 * off[c].  Position n, the $ suffix of row 0, belongs to no contig.  This is the convention of the read CSR: the
 * d_read_offsets that genie_reads_from_fasta writes for a reference file is a valid table as it is, its d_bases the
 * concatenation to build the index from (genie_index_create_device).
 * genie_contigs_validate checks the three conditions on the device, in one pass and one synchronisation of `stream` (as
 * genie_index_validate does for an image): GENIE_OK or GENIE_E_INVALID.  The calls below do NOT repeat the check.  They are
 * memory-safe on any table contents: a table that genie_contigs_validate would refuse gives undefined values, but no load
 * or store outside the declared sizes (the lookup bisects over the indices 0 .. n_contigs only and clamps what it derives).
 * In every call of this group a null ix, a null or not 8-byte aligned table or n_contigs < 1 gives GENIE_E_INVALID and
 * n_contigs above 2^31 - 2 GENIE_E_TOO_LONG, before the device check.
 * The lookup: a block stages samples of the table in LDS (every 2^shift-th offset, clamped, as int32) and a lane bisects
 * those, then the 2^shift entries between two of them in global memory: up to 1023 contigs from LDS alone, four L2 loads on
 * top at 10^4.  The walks of genie_find_mems_contigs stage up to 12 288 samples (48 KB) in blocks whose positions have that
 * many seed rows. */
int genie_contigs_validate(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, void *stream);

/* genie_find_mems on a reference of several sequences: the MEMs of a strand-read against the SET of contigs, i.e. the union
 * over c of its MEMs against contig c alone.  Arguments: those of genie_find_mems with the table behind ix.  Inputs, flags,
 * strands, breaks, d_status, max_occ, d_totals, the sizing call (d_rows == NULL), out_cap_rows and the synchronisations
 * (those of genie_match_stats and no more) are genie_find_mems's.  The definition changes in two places.  A MEM is (p, t, l)
 * with l >= m, Q[p .. p+l) == T[t .. t+l), no break inside, and it lies inside one contig: l <= room(t);
 *   right-maximal   p + l == L, or l == room(t), or Q[p+l] != T[t+l];
 *   left-maximal    p == 0, or t is a contig start, or Q[p-1] != T[t-1].
 * Rows stay int32 (start, end, pos, row): pos is 1-based IN THE CONCATENATION (genie_contig_coords names it), row the
 * suffix-array row of t, the order (start, row) within a strand-read, strand-reads in input order.  Every such MEM is found
 * from an occurrence of its seed Q[p .. p+m) in the concatenation: an occurrence with room(t) < m is no row, the
 * left-maximality rule gains the contig start, the length is clipped to room(t).  max_occ and GENIE_READ_ABSENT_BASE keep
 * referring to the concatenation: it is the seed's interval there, bridging occurrences included, that bounds the work.
 * Properties: with n_contigs == 1 the outputs are byte for byte those of genie_find_mems; the (start, end, pos) triples of a
 * strand-read are the union over c of what genie_find_mems gives on an index of contig c alone, pos shifted by off[c].
 * Checks: genie_find_mems's, then the table's (above), then the workspace's (GENIE_E_CAPACITY), all before the device
 * check.  The workspace function takes genie_find_mems_workspace_bytes's arguments and n_contigs; it returns
 * GENIE_E_INVALID for arguments the call would refuse, is a multiple of 256, monotone in N, total_bases and n_contigs, and
 * at least genie_find_mems_workspace_bytes of the same batch; what it adds is a function of n_contigs alone (today
 * nothing: the table is the caller's and its samples live in LDS).
 * Cost: genie_find_mems plus one lookup per seed occurrence, in the count and in the fill. */
int64_t genie_find_mems_contigs_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags, int64_t n_contigs);
int genie_find_mems_contigs(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t flags,
                            const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N, int64_t total_bases,
                            int64_t max_len, int32_t min_len, int32_t max_occ,
                            int64_t *d_offsets,      /* S * N + 1 */
                            int32_t *d_rows,         /* 4 * out_cap_rows, 16-byte aligned; may be NULL: counting only */
                            int64_t out_cap_rows,
                            int32_t *d_status,       /* S * N, may be NULL */
                            int64_t *d_totals,       /* 2, may be NULL: {rows in all, positions skipped by max_occ} */
                            void *d_workspace, int64_t workspace_bytes, void *stream);

/* SMEM rows -> hits named by contig, BWA's rule.  Input: S rows int32 (start, end, lo, hi), 16-byte aligned: the rows of any
 * genie_find_smems* call.  The rows stay SMEMs OF THE CONCATENATION -- this call does not make them SMEMs of the sequence
 * set --; it drops the occurrences that bridge two sequences.  For row j with len = end - start, every suffix-array row r in
 * [lo, hi] gives t = SA[r]; the hit is kept iff t < n and len <= room(t), and is the int32 pair (contig, 1-based offset
 * inside the contig); hits come out in row order.  An interval with lo < 0 or hi < lo contributes nothing.
 *   d_hit_offsets  S + 1 int64, 8-byte aligned: row j's hits are d_hits[2 off[j] .. 2 off[j+1]); [S] keeps the true total
 *   d_hits         2 * cap_hits int32, 8-byte aligned; may be NULL: the sizing call.  Hits past cap_hits are dropped.
 *   d_totals       2 int64, may be NULL: {hits kept, occurrences dropped as bridging}
 *   d_tmp          256-byte aligned scratch of genie_locate_contigs_tmp_bytes(S) bytes (GENIE_E_CAPACITY otherwise; the size
 *                  function gives GENIE_E_INVALID for S < 0 and a multiple of 256 else, monotone in S)
 * Count, scan and fill, one lane per interval up to 32 rows and the whole wave beyond; no atomic decides a value; no
 * synchronisation of `stream`. */
int64_t genie_locate_contigs_tmp_bytes(int64_t S);
int genie_locate_contigs(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, const int32_t *d_rows,
                         int64_t S, int64_t *d_hit_offsets, int32_t *d_hits, int64_t cap_hits, int64_t *d_totals, void *d_tmp,
                         int64_t tmp_bytes, void *stream);

/* 1-based concatenation positions d_pos[i * stride], i < count, -> d_out[2 i .. 2 i + 2) = (contig, 1-based offset inside
 * it); a position outside [1, n] gives (-1, -1).  Pass d_rows + 2 with stride 4 for MEM rows, a genie_locate result with
 * stride 1.  stride >= 1; d_pos and d_out 4-byte aligned.  One lane per element, no synchronisation of `stream`. */
int genie_contig_coords(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, const int32_t *d_pos,
                        int32_t stride, int64_t count, int32_t *d_out /* 2 * count */, void *stream);

/* Chain the MEM rows of every strand-read into collinear chains: candidate mapping locations with contig, strand (the unit)
 * and score, where genie_find_mems* stop.  The call consumes the rows exactly as those calls write them, ordered by (start, row)
 * within a strand-read: query order is a topological order of the recurrence, so nothing is sorted.  Everything is integer
 * and deterministic: the outputs are a function of the inputs alone.
 * Units.  A unit is one strand-read: the rows d_rows[4 off[u] .. 4 off[u+1]) of d_offsets[U + 1], as genie_find_mems* write
 * them.  Anchor i of a unit is the row (s_i, e_i, pos_i, row_i): l_i = e_i - s_i >= 1, t_i = pos_i - 1 with 0 <= t_i < n, s
 * non-decreasing in i; column 3 (row) is never read.  With a contig table (as genie_contigs_validate takes it) c_i is the
 * contig of t_i by that comment's rule; with d_contig_offsets == NULL and n_contigs == 0 every c_i is 0.  Rows that break
 * these assumptions give undefined values, but no load or store outside the declared sizes and no unbounded loop.
 * Parameters (int32): max_dist in [1, 2^22]; bandwidth in [0, max_dist]; gap_cost in [0, 255], in sixteenths of a base;
 * max_pred >= 0, 0 = no limit; min_score >= 0.  The call has no defaults.
 * Link.  j may precede i iff j < i; j >= i - max_pred when max_pred > 0; c_j == c_i; dq = s_i - s_j and dr = t_i - t_j both in
 * [1, max_dist]; g = |dr - dq| <= bandwidth; gain(j, i) = min(l_i, dq, dr) - ((g * gap_cost) >> 4) >= 1.
 * Recurrence.  f(i) = max(l_i, max over linkable j of f(j) + gain(j, i)); p(i) is the largest j that attains that maximum
 * if the maximum is strictly greater than l_i, else -1.  f rises strictly along every link.
 * Chains.  The p links form a forest.  top(i) is the node of i's subtree, i included, with the largest (f, then smallest
 * index); one chain is the set of anchors with the same top: a path that ends in a leaf, and every leaf is the top of exactly
 * one chain.  (minimap2's extraction: visit anchors by (f descending, index ascending), backtrack until a used anchor.)
 * Score.  With v the chain's top and u its first anchor: f(v) - f(p(u)) if p(u) >= 0, else f(v).  A chain is kept iff its
 * score >= min_score.
 * Outputs, all in caller buffers:
 *   d_chain_offsets  U + 1 int64, 8-byte aligned: the offsets of each unit's kept chains; [U] is the true total even when
 *                    cap_chains is smaller
 *   d_chains         8 int32 per chain, 16-byte aligned, may be NULL (the sizing call): (q_begin, q_end, r_begin, r_end, score,
 *                    n_anchors, contig, last) with q_begin = s_u, r_begin = pos_u (1-based in the concatenation), q_end the
 *                    largest e and r_end the largest pos + l over the members, last = v's row index inside its unit.  The
 *                    chains of a unit are ordered by last ascending; chains past cap_chains are dropped.
 *   d_anchor_chain   total_rows int32, may be NULL: the index of the anchor's chain inside its unit (whether or not that chain
 *                    fits cap_chains), -1 if that chain was not kept
 *   d_anchor_pred    total_rows int32, may be NULL: p(i) inside the unit
 *   d_anchor_score   total_rows int32, may be NULL: f(i)
 *   d_totals         2 int64, 8-byte aligned, may be NULL: {chains kept, chains not kept}
 * Anchors at or past off[U] are left untouched.  No atomic decides a value.
 * total_rows is the host-side bound: the size of d_rows and of the anchor arrays.  The device checks off[0] == 0, off
 * non-decreasing, off[U] <= total_rows and no unit above 2^31 - 1 rows: GENIE_E_INVALID, found on the device, at the cost of
 * the call's only synchronisation of `stream`.
 * Checked before that and before the device check, so on any handle, GENIE_E_INVALID: a null ix, d_offsets or
 * d_chain_offsets; a null d_rows with total_rows > 0; a negative size; a parameter outside its range; d_rows or d_chains not
 * 16-byte, d_offsets, d_chain_offsets, d_totals or the table not 8-byte, an anchor array not 4-byte aligned; a table with
 * n_contigs < 1 or a null table with n_contigs != 0 (GENIE_E_TOO_LONG for n_contigs above 2^31 - 2).  Then, for U > 0, a
 * d_workspace that is null, not 256-byte aligned or smaller than genie_chain_mems_workspace_bytes(U, total_rows, n_contigs)
 * gives GENIE_E_CAPACITY.  U == 0 writes d_chain_offsets[0] = 0 and zero totals.
 * The workspace function returns GENIE_E_INVALID for negative arguments, is a multiple of 256 and monotone in U and
 * total_rows: 24 bytes per row (f 4, p 4, top 4, kept flag 4, the key handed up between chunks 8), 28 with more than one
 * contig (the anchor's contig), 8 bytes per unit (chains kept, chains in all) and 8 per 1024 units (the scan).
 * Kernels: one wave per unit, the unit's last kChainTile = 512 anchors as (s, t, c, f) in an LDS ring, 64 lanes over the
 * window's candidates and a wave max-reduce per anchor; older candidates come from the workspace.  Cost: per anchor its
 * window's candidates / 64 steps, so max_pred bounds the work on repeat-rich rows; a unit is not split, so one unit of very
 * many rows runs on one wave. */
int64_t genie_chain_mems_workspace_bytes(int64_t U, int64_t total_rows, int64_t n_contigs);
int genie_chain_mems(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs,
                     const int64_t *d_offsets,        /* U + 1 */
                     const int32_t *d_rows,           /* 4 * total_rows, 16-byte aligned */
                     int64_t U, int64_t total_rows,
                     int32_t max_dist, int32_t bandwidth, int32_t gap_cost, int32_t max_pred, int32_t min_score,
                     int64_t *d_chain_offsets,        /* U + 1 */
                     int32_t *d_chains,               /* 8 * cap_chains, 16-byte aligned; may be NULL: sizing only */
                     int64_t cap_chains,
                     int32_t *d_anchor_chain,         /* total_rows, may be NULL */
                     int32_t *d_anchor_pred,          /* total_rows, may be NULL */
                     int32_t *d_anchor_score,         /* total_rows, may be NULL */
                     int64_t *d_totals,               /* 2, may be NULL: {chains kept, chains not kept} */
                     void *d_workspace, int64_t workspace_bytes, void *stream);

/* Align every chain: a banded affine gap fill between the members of a chain and a banded extension at both ends, where
 * genie_chain_mems stops.  A chain's score is an estimate from anchor lengths; this call looks at the bases between the anchors
 * and beyond the first and the last.  Score and end points only: no traceback, no CIGAR.  Everything is integer and
 * deterministic: the outputs are a function of the inputs alone.
 * Inputs.
 *   reads    d_bases, d_read_offsets, N, total_bases, max_len, flags exactly as genie_find_mems* take them.
 *            GENIE_READS_BOTH_STRANDS gives S = 2 (else 1); unit u = S i + s is read i on strand s, of length L.  On strand 1
 *            the query Q is the reverse complement, built on the fly: position p is 3 - bases[o + L - 1 - p], and a code > 3
 *            stays what it is.  GENIE_READS_SPLIT_BREAKS is accepted and changes nothing; any other bit: GENIE_E_INVALID.
 *   anchors  d_offsets[U + 1], d_rows, total_rows: the MEM rows as genie_find_mems* wrote them; U must equal S N
 *            (GENIE_E_INVALID).  d_anchor_chain and d_anchor_pred as genie_chain_mems wrote them: both are required.
 *   chains   d_chain_offsets[U + 1], d_chains, cap_chains as genie_chain_mems wrote them.  The chains with global index
 *            c < C = min(d_chain_offsets[U], cap_chains) are aligned.
 *   contigs  d_contig_offsets, n_contigs as genie_chain_mems takes them; NULL with n_contigs == 0: one contig [0, n).  The
 *            chain's contig is column 6 of its row; its bounds [clo, chi) are two reads of the table.
 *   T        the reference: the packed 2-bit bases of the image.
 * Parameters (int32; the call has no defaults): match a in [1, 64]; mismatch b in [0, 64]; gap_open o in [0, 64]; gap_extend e
 * in [1, 64]; band w in [0, 511]; max_indel in [0, 1023 - 2 w]; end_bonus in [0, 32768].  A gap of g bases costs o + g e.  No
 * dynamic program is wider than 2 w + max_indel + 1 <= GENIE_ALIGN_MAX_DIAGS diagonals.  Anything outside its range gives
 * GENIE_E_INVALID.  Scores fit an int32: (2 max_len + max_indel + 2 w + 2) max(a, b, o + e) + 2 end_bonus < 2^30, else
 * GENIE_E_TOO_LONG.
 * Base score.  s(x, y) = a if x == y and x <= 3, else -b: a break of the query (a code > 3) is a mismatch against everything.
 * Banded affine dynamic program.  For strings x[0 .. A), y[0 .. B) and the diagonals d = j - i in [dlo, dhi]: cells outside
 * the rectangle or outside the band are -infinity; H(0, 0) = 0;
 *   E(i, j) = max(H(i, j-1) - o - e, E(i, j-1) - e);  F(i, j) = max(H(i-1, j) - o - e, F(i-1, j) - e);
 *   H(i, j) = max(H(i-1, j-1) + s(x_i, y_j), E(i, j), F(i, j)).
 * Members.  The members of chain c of unit u are found by starting at row `last` (column 7 of the chain row) and following
 * d_anchor_pred while d_anchor_chain equals c - d_chain_offsets[u].  Their starts s and reference positions t = pos - 1 rise
 * strictly; their length is l = e - s.
 * Trimming, from the last member backwards.  cur = (qs, ts) = (s, t) of the last member, which is used whole.  For each
 * earlier member j, in descending order: ov = max(0, s_j + l_j - qs, t_j + l_j - ts) and l' = l_j - ov.  If l' <= 0 member j is
 * skipped.  Otherwise the gap is A = qs - (s_j + l'), B = ts - (t_j + l'), both >= 0.  If |B - A| > max_indel the chain is
 * SKIPPED: flag bit 4 is set and every other column is 0.  Otherwise a l' + gapfill is added and cur = (s_j, t_j).  gapfill is
 * H(A, B) of the dynamic program on Q[s_j + l' .. qs) and T[t_j + l' .. ts) with the band [min(0, B - A) - w, max(0, B - A) + w].
 * Extension of x[0 .. A) against y, where y is cut to its first A + w bases and B is its length, with the band [-w, w]: M is
 * the largest H over all cells (>= 0, because H(0, 0) = 0), taken at the cell with the smallest i + j and among those the
 * smallest i.  If row A has a cell inside the band and the rectangle, G = max_j H(A, j), taken at the smallest such j.  If
 * G + end_bonus >= M the extension is TO THE END: its value is G + end_bonus and it consumes (A, j_G); a tie goes to the end;
 * with A = 0 this rule gives the value end_bonus.  Otherwise the extension is local: its value is M at (i*, j*).
 * Where the extensions run.  Right: x = Q[e_last .. L), y = T[t_last + l_last .. chi).  Left: x = Q[0 .. qs) reversed,
 * y = T[clo .. ts) reversed, with (qs, ts) the start of the first used member.
 * Output.  d_aln: 8 int32 per chain, 16-byte aligned, parallel to d_chains:
 *   (score, q_begin, q_end, r_begin, r_end, flags, n_used, matched)
 * score is the sum of the members' a l', the gap fills and both extensions; [q_begin, q_end) is the aligned part of the
 * strand-read; r_begin and r_end are 1-based in the concatenation, as in chain rows, r_end one past the last base; flags bit 1:
 * the left extension went to the read's start, bit 2: the right extension went to the read's end, bit 4: the chain was
 * skipped; n_used is the number of members not skipped by trimming; matched is the sum of l'.  d_totals (2 int64, may be
 * NULL): {chains aligned, chains skipped}.  Rows of d_aln at or past C are left untouched.  No atomic decides a value.
 * Rows, chain rows and anchor arrays that break the assumptions give undefined values, but no load or store outside the
 * declared sizes and no unbounded loop: the walk is bounded by the unit's row count, positions are clamped to [0, L] and
 * [clo, chi), a contig or unit index to its table.
 * Checked before the device check, so on any handle, GENIE_E_INVALID: a null ix, d_offsets or d_chain_offsets; null bases or
 * read offsets where there are reads; a null d_rows, d_anchor_chain or d_anchor_pred with total_rows > 0; a null d_chains or
 * d_aln with cap_chains > 0; a negative size; U != S N; a flag or parameter outside its range; d_rows, d_chains or d_aln not
 * 16-byte, an offsets array, d_totals or the table not 8-byte, an anchor array not 4-byte aligned; a table with n_contigs < 1
 * or a null table with n_contigs != 0 (GENIE_E_TOO_LONG for n_contigs above 2^31 - 2).  Then GENIE_E_TOO_LONG as above.  Then,
 * for U > 0, a d_workspace that is null, not 256-byte aligned or smaller than genie_align_chains_workspace_bytes(U, cap_chains)
 * gives GENIE_E_CAPACITY.  Then GENIE_E_NO_DEVICE.  The read offsets and the row offsets are checked on the device as
 * genie_find_mems* and genie_chain_mems check them (GENIE_E_INVALID), at the cost of the call's only synchronisation of
 * `stream`.  U == 0 or C == 0 writes zero totals and nothing else.
 * The workspace function returns GENIE_E_INVALID for negative arguments, is a multiple of 256 and monotone in both: 4 bytes
 * per chain (the chain's unit), 0 bytes per unit, and 256 for the verdict of the offset checks.
 * Kernels: one wave per chain, lanes over the band's diagonals and rows over the query's bases, the row before in LDS (8 bytes
 * per diagonal), bands of more than 64 diagonals in chunks of 64.  Cost: per gap and per end, rows x ceil(diagonals / 64)
 * steps; a chain is not split, so one chain with very long gaps runs on one wave. */
#define GENIE_ALIGN_MAX_DIAGS 1024
int64_t genie_align_chains_workspace_bytes(int64_t U, int64_t cap_chains);
int genie_align_chains(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t flags,
                       const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N, int64_t total_bases, int64_t max_len,
                       const int64_t *d_offsets,        /* U + 1 */
                       const int32_t *d_rows,           /* 4 * total_rows, 16-byte aligned */
                       int64_t U, int64_t total_rows,
                       const int32_t *d_anchor_chain,   /* total_rows */
                       const int32_t *d_anchor_pred,    /* total_rows */
                       const int64_t *d_chain_offsets,  /* U + 1 */
                       const int32_t *d_chains,         /* 8 * cap_chains, 16-byte aligned */
                       int64_t cap_chains,
                       int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, int32_t band, int32_t max_indel,
                       int32_t end_bonus,
                       int32_t *d_aln,                  /* 8 * cap_chains, 16-byte aligned */
                       int64_t *d_totals,               /* 2, may be NULL: {chains aligned, chains skipped} */
                       void *d_workspace, int64_t workspace_bytes, void *stream);

/* The CIGAR of selected chains: the traceback of genie_align_chains, where that call stops at score and end points.  The call
 * takes everything genie_align_chains takes, with the same parameters, ranges and checks, the rows d_aln as that call wrote
 * them, and a selection.  Everything is integer and deterministic: the outputs are a function of the inputs alone.
 * Selection.  d_sel: n_sel int64 global chain indices, 8-byte aligned.  NULL: the chains 0 .. C - 1 in order, C =
 * min(d_chain_offsets[U], cap_chains); n_sel is then ignored and taken as C (the outputs hold C entries, the workspace is that of
 * n_sel = cap_chains).  An index may occur more than once: its results are repeated.  An index outside [0, C) gives a flagged,
 * empty result (bit 16), not an error.
 * Pieces.  The alignment of a chain is cut into pieces in forward strand-read order: the left extension; then, alternately, a
 * used member's l' bases and the gap fill behind it; the last member whole; the right extension.  Members, trimming, l', the
 * gaps (A, B) and their bands are exactly those of genie_align_chains.  A member is l' ops '='.  A gap fill is the canonical
 * path (below) of the same program from (A, B) back to (0, 0).  An extension is the canonical path of the GLOBAL program
 * between (0, 0) and the cell (i*, j*) the extension consumed, on the rectangle [0, i*] x [0, j*] with the band [-w, w]; the cell
 * is read off d_aln:
 *   right: i* = q_end - e_last,  j* = (r_end - 1) - (t_last + l_last);
 *   left:  i* = qs - q_begin,    j* = ts - (r_begin - 1), on the reversed strings.
 * The program is causal, so H(i*, j*) of this rectangle is the value the extension found.  i* = 0 forces j* = 0 and gives no
 * ops.  An end cell outside the band or outside the extension's rectangle [0, A] x [0, B], or with i* = 0 < j*, flags the chain
 * (bit 16, no ops).  Rows of d_aln that genie_align_chains did not write give undefined values but, like every other input
 * here, no access outside the declared sizes and no unbounded loop: the end cells are checked before they are used, and a
 * trace takes at most i + j steps whatever it reads.
 * The canonical path is defined on the values H / E / F above, from the piece's end cell backwards.
 *   State H at (i, j): stop at (0, 0).  Otherwise the first that holds: (1) i, j >= 1, (i-1, j-1) inside band and rectangle and
 *   H(i, j) == H(i-1, j-1) + s(x_i, y_j): emit '=' if x_i == y_j and x_i <= 3, else 'X', go to H at (i-1, j-1); (2) H(i, j) ==
 *   F(i, j): go to state F; (3) else go to state E.
 *   State F (consumes query): emit 'I' and move to (i-1, j); stay in F iff F(i, j) == F(i-1, j) - e, with (i, j) the cell before
 *   the move; otherwise the state is H.  A tie between opening and extending goes to extending.
 *   State E (consumes reference): emit 'D' and move to (i, j-1); stay in E iff E(i, j) == E(i, j-1) - e; otherwise H.
 * The order is diagonal, F, E, and extend before open: the order in which the kernel's recurrence compares.  A path from a
 * finite cell only meets finite cells.  The closed forms of genie_align_chains are this path: A = 0 or B = 0 is one 'D' or one
 * 'I' of A + B bases, A = B = 0 is nothing.  The ops of a piece are emitted from its end cell backwards and reversed; the left
 * extension runs on reversed strings, so its ops come out in strand-read order as they are emitted.
 * Ops.  An op is SAM's uint32 len << 4 | op with I = 1, D = 2, S = 4, '=' = 7, X = 8 (len < 2^28).  Neighbouring equal ops
 * are merged across piece borders.  A leading S of q_begin bases and a trailing S of L - q_end bases are written when non-zero.
 * The ops are in strand-read order: on strand 1 that of the reverse complement, SAM's convention.  A query code above 3 is
 * always 'X'.
 * Outputs, all in caller buffers:
 *   d_cigar_offsets  n_sel + 1 int64, 8-byte aligned; [n_sel] holds the true total even when cap_ops is smaller
 *   d_cigar          cap_ops uint32, 4-byte aligned; NULL is the sizing call.  Ops past cap_ops are dropped.
 *   d_info           8 int32 per selected chain, 16-byte aligned:
 *                    (chain, flags, n_ops, nm, n_eq, n_x, ins_bases, del_bases), nm = n_x + ins_bases + del_bases.  Flag bit
 *                    4: the chain was skipped by genie_align_chains; bit 8: no room for its directions; bit 16: bad index or
 *                    end cell.  Any flag set means n_ops = 0 and the other columns 0.
 *   d_dir_need       n_sel int64, 8-byte aligned, may be NULL: the direction bytes each selected chain needs
 *   d_totals         3 int64, 8-byte aligned, may be NULL: {chains written, chains flagged, direction bytes needed in all}
 * Outputs past n_sel and past the true op total are left untouched.  No atomic decides a value.
 * Direction storage.  Every cell of a piece with A >= 1 and B >= 1 keeps four bits: bits 0-1 the source of H (0 diagonal and
 * '=', 1 diagonal and 'X', 2 F, 3 E), bit 2: F(i, j) == F(i-1, j) - e, bit 3: E(i, j) == E(i, j-1) - e.  A piece of A rows on D
 * diagonals takes A * ceil(D / 64) * 32 bytes: row i - 1, two diagonals to a byte, the even one in the low half.  Pieces in
 * closed form take nothing.  The need of a chain is the sum over its pieces, a function of its geometry alone (members, gaps
 * and end points); a flagged chain needs 0.  The storage is dir_bytes of the workspace, the caller's budget: selected chain k
 * gets room iff the running sum of the needs through k is at most dir_bytes; the others get bit 8, and d_totals[2] tells what to
 * come back with.
 * Checks: all those of genie_align_chains up to its alignment and table checks, in that order (d_aln is required whatever
 * cap_chains is, and is read only); then GENIE_E_INVALID for a null d_aln, d_cigar_offsets or d_info, a negative n_sel, cap_ops
 * or dir_bytes, a d_sel, d_cigar_offsets, d_dir_need not 8-byte, d_info not 16-byte or d_cigar not 4-byte aligned; then
 * GENIE_E_TOO_LONG as there; then, for U > 0 or a selection, a d_workspace that is null, not 256-byte aligned or smaller than
 * genie_chain_cigars_workspace_bytes(U, cap_chains, n_sel, dir_bytes) gives GENIE_E_CAPACITY; then GENIE_E_NO_DEVICE.  The read
 * offsets and the row offsets are checked on the device as there (GENIE_E_INVALID), at the cost of the call's only
 * synchronisation of `stream`.  No selected chain: d_cigar_offsets[0] = 0 and zero totals.
 * The workspace function returns GENIE_E_INVALID for negative arguments, is a multiple of 256 and monotone in all four: 4 bytes
 * per chain (the chain's unit), 20 bytes per selected chain (op count 4, need 8, direction offset 8) and 8 per 1024 of them (the
 * scan), 0 bytes per unit, dir_bytes rounded up to 256, and 256 for the verdict of the offset checks.
 * Kernels: a plan (one lane per selected chain: the need), one block for the running sum, the fill (one wave per selected
 * chain, genie_align_chains' program with one 4-bit store per cell), and the trace (one lane per selected chain, one step per
 * op base), run twice: it counts, the offsets are scanned, it writes. */
int64_t genie_chain_cigars_workspace_bytes(int64_t U, int64_t cap_chains, int64_t n_sel, int64_t dir_bytes);
int genie_chain_cigars(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t flags,
                       const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N, int64_t total_bases, int64_t max_len,
                       const int64_t *d_offsets,        /* U + 1 */
                       const int32_t *d_rows,           /* 4 * total_rows, 16-byte aligned */
                       int64_t U, int64_t total_rows,
                       const int32_t *d_anchor_chain,   /* total_rows */
                       const int32_t *d_anchor_pred,    /* total_rows */
                       const int64_t *d_chain_offsets,  /* U + 1 */
                       const int32_t *d_chains,         /* 8 * cap_chains, 16-byte aligned */
                       int64_t cap_chains,
                       int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, int32_t band, int32_t max_indel,
                       int32_t end_bonus,
                       const int32_t *d_aln,            /* 8 * cap_chains, 16-byte aligned: as genie_align_chains wrote it */
                       const int64_t *d_sel,            /* n_sel, may be NULL: every chain */
                       int64_t n_sel,
                       int64_t *d_cigar_offsets,        /* n_sel + 1 */
                       uint32_t *d_cigar,               /* cap_ops, may be NULL: sizing only */
                       int64_t cap_ops,
                       int32_t *d_info,                 /* 8 * n_sel, 16-byte aligned */
                       int64_t *d_dir_need,             /* n_sel, may be NULL */
                       int64_t *d_totals,               /* 3, may be NULL */
                       int64_t dir_bytes,
                       void *d_workspace, int64_t workspace_bytes, void *stream);

/* The alignments of every read: which of its chains, as genie_align_chains scored them, are its primary, its supplementary
 * and its secondary alignments, each with a mapping quality; the selection goes straight into genie_chain_cigars as d_sel.
 * Everything is integer and deterministic.  The rule is minimap2's parent rule and the quality minimap2's shape without the
 * logarithm: a POLICY, expressed through five scalars, not a model.
 * Inputs, all as the earlier calls wrote them:
 *   reads    d_read_offsets[N + 1], N: used for the read lengths L alone.
 *   flags    GENIE_READS_BOTH_STRANDS: S = 2 strand-reads per read, unit 2 i + 1 the reverse complement of read i; otherwise
 *            S = 1.  GENIE_READS_SPLIT_BREAKS is accepted and changes nothing; any other bit: GENIE_E_INVALID.
 *   chains   d_chain_offsets[U + 1] with U == S N (GENIE_E_INVALID), d_chains (only column 6, the contig, is read), d_aln,
 *            cap_chains.  C = min(d_chain_offsets[U], cap_chains).
 *   contigs  d_contig_offsets, n_contigs as genie_align_chains takes them; NULL with n_contigs == 0: one contig [0, n).
 * Parameters (int32; the call has no defaults): mask_level in [0, 100]; pri_ratio in [0, 100]; max_secondary in [0, 2^20];
 * min_score in [1, 2^30]; mapq_full in [1, 2^20].  Anything outside its range gives GENIE_E_INVALID.
 * Candidates.  The candidates of read i are the chains c < C of its units S i .. S i + S - 1 whose d_aln row has flag bit 4
 * clear and score >= min_score.
 * Query interval.  A candidate's interval is taken in FORWARD read coordinates: on strand 0 [q_begin, q_end), on strand 1
 * [L - q_end, L - q_begin); both ends are clamped to [0, L].  Its length is end - begin.
 * Key order.  (score descending, global chain index ascending): a tie goes to the smaller chain index.
 * Overlap.  Two candidates of a read overlap iff 100 ov > mask_level min(len_i, len_j) in 64-bit arithmetic, ov the length of
 * the intersection of their forward intervals.  Equality is no overlap.  Strand and contig play no part.
 * Classification.  Walk the candidates of a read in key order.  A candidate that overlaps no earlier primary is a primary.
 * Otherwise it is a secondary, and its parent is the first primary in key order that it overlaps.  The read's first primary
 * has kind 0, later primaries kind 1 (supplementary), secondaries kind 2, chains c < C that are no candidate kind 3.
 * Per primary P: n_sec(P) is the number of its secondaries, sub(P) the largest score among them (0 if none), and
 *   mapq(P) = floor(60 (score - min(sub, score)) min(matched, mapq_full) / (score mapq_full))
 * in int64, matched being column 7 of d_aln (taken as 0 when negative): a value in [0, 60].  A secondary has mapq 0.
 * Selection of a read: first its primaries in key order; then the ELIGIBLE secondaries in key order, at most max_secondary of
 * them.  A secondary is eligible iff 100 score >= pri_ratio score(parent).  Equality is eligible.
 * Outputs, all in caller buffers:
 *   d_class        4 int32 per chain, 16-byte aligned, parallel to d_aln, written for every c < C:
 *                  (kind, parent, order, mapq).  parent is the global chain index of its primary, a primary its own, -1 for
 *                  kind 3; order is its index inside its read's selection, -1 if not selected.  Rows at or past C are left
 *                  untouched.
 *   d_sel_offsets  N + 1 int64, 8-byte aligned; [N] holds the true total even when cap_sel is smaller
 *   d_sel          cap_sel int64 global chain indices, 8-byte aligned, in the order above; NULL is the sizing call.  Entries
 *                  past cap_sel are dropped.
 *   d_records      12 int32 per selected chain, 16-byte aligned, parallel to d_sel; may be NULL only together with d_sel:
 *                  (read, chain, kind, strand, contig, offset, r_span, q_begin, q_end, score, sub, mapq)
 *                  offset is the 1-based start inside the contig, r_begin - d_contig_offsets[contig], and r_begin itself (and
 *                  contig 0) without a table; r_span = r_end - r_begin; q_begin and q_end are in forward read coordinates;
 *                  sub is 0 for a secondary.
 *   d_read_counts  4 int32 per read, 16-byte aligned, may be NULL: (candidates, primaries, secondaries, best chain or -1)
 *   d_totals       4 int64, 8-byte aligned, may be NULL: {candidates, primaries, secondaries, selected}; it stays on the device
 * No atomic decides a value: the outputs are a function of the inputs alone.  d_aln or chain rows that break the assumptions
 * give undefined values, but no load or store outside the declared sizes and no unbounded loop: the contig index is clamped to
 * the table, positions are clamped to [0, L], and the rounds of a read are bounded by its chain count.
 * Checked before the device check, so on any handle, GENIE_E_INVALID: a null ix, d_chain_offsets or d_sel_offsets; null read
 * offsets where there are reads; a null d_chains, d_aln or d_class with cap_chains > 0; a d_sel without d_records; a negative
 * size; a flag outside the two; U != S N; a parameter outside its range; d_chains, d_aln, d_class, d_records or d_read_counts not
 * 16-byte, an offsets array, d_sel, d_totals or the table not 8-byte aligned; a table with n_contigs < 1 or a null table with
 * n_contigs != 0 (GENIE_E_TOO_LONG for n_contigs above 2^31 - 2).  Then GENIE_E_TOO_LONG for N or cap_chains above 2^31 - 1:
 * reads and chains are named by an int32.  Then, for U > 0, a d_workspace that is null, not 256-byte aligned or smaller than
 * genie_select_alignments_workspace_bytes(N, cap_chains) gives GENIE_E_CAPACITY.  Then GENIE_E_NO_DEVICE.  The chain offsets are
 * checked on the device as genie_align_chains checks its row offsets (GENIE_E_INVALID), at the cost of the call's only
 * synchronisation of `stream`.  U == 0 or C == 0 writes zero offsets and zero totals (and, for U > 0, the counts of every read).
 * The workspace function returns GENIE_E_INVALID for negative arguments, is a multiple of 256 and monotone in both: 4 bytes
 * per chain (sub of a primary), 64 bytes per read (its counts 16, its selected count 4, the wide mark 4, its row in the list of
 * wide reads twice 16, that list's offset 8) and 8 per 1024 reads (the scan), and 256 for the verdict of the offset check.
 * Kernels: greedy rounds, which give the walk's result without a sort: the best unassigned candidate (an arg-max over a packed
 * 64-bit key) becomes a primary and takes every unassigned candidate that overlaps it; the selected secondaries are further
 * arg-max rounds.  A read of at most GENIE_SELECT_LANE_MAX chains is run by one lane; the others are compacted into a list and
 * run one wave each, the state of their first GENIE_SELECT_TILE chains in LDS and that of the rest in d_class.  Cost of a read
 * of c chains with p primaries: about (p + max_secondary) ceil(c / 64) wave steps. */
#define GENIE_SELECT_LANE_MAX 8
#define GENIE_SELECT_TILE 512
int64_t genie_select_alignments_workspace_bytes(int64_t N, int64_t cap_chains);
int genie_select_alignments(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t flags,
                            const int64_t *d_read_offsets,  /* N + 1 */
                            int64_t N,
                            const int64_t *d_chain_offsets, /* U + 1 */
                            int64_t U,
                            const int32_t *d_chains,        /* 8 * cap_chains, 16-byte aligned */
                            const int32_t *d_aln,           /* 8 * cap_chains, 16-byte aligned: as genie_align_chains wrote it */
                            int64_t cap_chains,
                            int32_t mask_level, int32_t pri_ratio, int32_t max_secondary, int32_t min_score, int32_t mapq_full,
                            int32_t *d_class,               /* 4 * cap_chains, 16-byte aligned */
                            int64_t *d_sel_offsets,         /* N + 1 */
                            int64_t *d_sel,                 /* cap_sel, may be NULL: sizing only */
                            int32_t *d_records,             /* 12 * cap_sel, 16-byte aligned; NULL only with d_sel */
                            int64_t cap_sel,
                            int32_t *d_read_counts,         /* 4 * N, 16-byte aligned, may be NULL */
                            int64_t *d_totals,              /* 4, may be NULL */
                            void *d_workspace, int64_t workspace_bytes, void *stream);

/* The alignments of paired-end reads: for every pair of mates, which of their candidate records of genie_select_alignments go
 * together, a pair mapping quality, and SAM's per-record fields (flag, mapq, mate, template length) of every record.
 * Everything is integer and deterministic: a POLICY, expressed through eight scalars, not a model.
 * Inputs:
 *   ix       used for the device and the launch sizes, as genie_select_alignments uses it.
 *   N        the number of reads, even (GENIE_E_INVALID otherwise); P = N / 2.  Mate m in {0, 1} of pair k is read 2 k + m: the
 *            interleaved convention, as GENIE_TEXT_FASTQ gives it on an interleaved file.
 *   records  d_sel_offsets[N + 1], d_records (12 int32 per record) and n_records: genie_select_alignments' outputs.
 *            R = min(d_sel_offsets[N], n_records); only records j < R exist for this call.
 *   class    d_class (4 int32 per chain) and cap_chains as genie_select_alignments wrote them.  Only column 1 (parent) is read,
 *            at index records[j].chain clamped to [0, cap_chains); with cap_chains == 0 no secondary is a candidate.
 * No contig table is needed: a record carries its contig and its 1-based offset inside it.
 * Parameters (int32; the call has no defaults): orient in [1, 7]: bit 0 FR, bit 1 RF, bit 2 same strand; isize_min, isize_max,
 * isize_mean each in [0, 2^30] with isize_min <= isize_max; pen_slope in [0, 65536]; pen_max in [0, 2^20]; pen_unpaired in
 * [0, 2^20]; mapq_boost in [0, 60].  Anything outside its range gives GENIE_E_INVALID.
 * Candidates.  The records of read r are the rows [so[r], so[r + 1]) of d_sel_offsets cut to [0, R); its HEAD is the first of
 * them, after genie_select_alignments the kind-0 primary.  A record is a candidate iff it is the head, or it has kind 2 and
 * d_class[chain].parent equals the head's chain.  Supplementary records (kind 1) and secondaries of a supplementary are never
 * candidates.  For a record: b = offset - 1, e = b + r_span, s = strand, w = score.
 * Combination.  A candidate x of mate 0 with a candidate y of mate 1.  Without the same contig the combination has no type.
 * span = max(e_x, e_y) - min(b_x, b_y).  With opposite strands, f the strand-0 record and r the strand-1 record, the type is
 * the first that holds of: f.b <= r.b and f.e <= r.e: FR (0); r.b <= f.b and r.e <= f.e: RF (1); otherwise (one strictly inside
 * the other) none (3).  With equal strands the type is "same" (2).  A combination is CONCORDANT iff its type's bit is set in
 * orient (type 3 never is) and isize_min <= span <= isize_max.  Its value is
 *   W = w_x + w_y - min(pen_max, floor(|span - isize_mean| pen_slope / 256))
 * in int64; stored columns are clamped to the int32 range.
 * Decision per pair.  W1 is the value of the best concordant combination, the key order being (W descending, x's record index
 * ascending, y's ascending); W2 the largest W among the OTHER concordant combinations, 0 when there is none; with both heads
 * present U = w(head 0) + w(head 1) - pen_unpaired.  The pair is PROPER iff both mates have records, a concordant combination
 * exists and W1 >= U.  Equality is proper.  For a proper pair the CHOSEN record of each mate is x*, y* of the best combination and
 *   pair_mapq = 0 if W1 <= 0, else floor(60 (W1 - min(max(W2, U, 0), W1)) / W1).
 * Otherwise the chosen record of a mate that has records is its head; a mate without records has none (-1).
 * Outputs, all in caller buffers:
 *   d_pairs   8 int32 per pair, 16-byte aligned: (rec0, rec1, flags, pair_score, sub_score, isize, n_concordant, type)
 *             rec0, rec1: the global record indices of the chosen records, or -1.  flags: bit 1 proper; bit 2 mate 0 has
 *             records; bit 4 mate 1 has records; bit 8 mate 0's chosen record is not its head; bit 16 the same for mate 1.
 *             pair_score = W1 when a concordant combination exists, else 0; sub_score = W2; isize and type: the span and type of
 *             the two chosen records when both exist and share a contig, otherwise 0 and -1; n_concordant clamped to int32.
 *   d_sam     4 int32 per record, 16-byte aligned, parallel to d_records, written for every j < R:
 *             (flag, mapq, mate_record, tlen)
 *             flag, in SAM's bits: 0x1 always; 0x2 on every record of a proper pair; 0x8 the mate has no chosen record; 0x10 the
 *             record's strand is 1; 0x20 the mate's chosen record exists and has strand 1; 0x40 / 0x80 mate 0 / mate 1; 0x800
 *             kind 1; 0x100 every record that is neither chosen nor kind 1 (a displaced head is one of those).
 *             mapq: a chosen record of a proper pair max(q, min(pair_mapq, q + mapq_boost)), q its own mapq column clamped to
 *             [0, 60]; a chosen record otherwise q; kind 1 its own; all others 0.
 *             mate_record: the mate's chosen record, or -1.
 *             tlen: 0 unless mate_record >= 0 and the contigs agree; then the span of this record and the mate's chosen one,
 *             positive if this record's b is smaller, negative if larger, at equal b positive for mate 0 and negative for mate 1.
 *             Rows at or past R are left untouched.
 *   d_totals  4 int64, 8-byte aligned, may be NULL: {pairs with both mates mapped, proper pairs, mates whose chosen record is not
 *             their head, pairs with exactly one mate mapped}; it stays on the device
 * No atomic decides a value: the outputs are a function of the inputs alone.  Garbage records or class rows give undefined
 * values, but no access outside the declared sizes and no unbounded loop: the record ranges are clamped to [0, R] and ordered,
 * the chain index is clamped, and a pair's work is bounded by the product of its record counts.
 * Checked before the device check, so on any handle, GENIE_E_INVALID: a null ix, d_sel_offsets or d_pairs; an odd or negative N,
 * a negative size; a null d_records or d_sam with n_records > 0; a null d_class with cap_chains > 0; a parameter outside its
 * range; d_records, d_class, d_pairs or d_sam not 16-byte, d_sel_offsets or d_totals not 8-byte aligned.  Then GENIE_E_TOO_LONG
 * for N or n_records above 2^31 - 1: reads and records are named by an int32.  Then, for N > 0, a d_workspace that is null, not
 * 256-byte aligned or smaller than genie_pair_alignments_workspace_bytes(N, n_records) gives GENIE_E_CAPACITY.  Then
 * GENIE_E_NO_DEVICE.  The record offsets are checked on the device as genie_select_alignments checks its chain offsets
 * (GENIE_E_INVALID), at the cost of the call's only synchronisation of `stream`.  N == 0 writes zero totals and nothing else.
 * The workspace function returns GENIE_E_INVALID for negative arguments, is a multiple of 256 and monotone in both: 48 bytes per
 * pair (the wide mark 4, its mapping quality 4, its row in the list of wide pairs twice 16, that list's offset 8) and 8 per 1024
 * pairs (the scan), each piece rounded up to 256 on its own, and 256 for the verdict of the offset check; nothing per record.
 * Kernels: a pair whose record counts multiply to at most GENIE_PAIR_LANE_MAX is decided by one lane; the others are compacted
 * into a list and run one wave each, lanes over the flattened combinations, the values of the first GENIE_PAIR_TILE records of
 * each mate in LDS and those beyond read from d_records; the best combination is an arg-max reduction, W2 one more over each
 * lane's two largest values; then one lane per record writes its d_sam row.  Cost of a pair of a x b records: about
 * ceil(a b / 64) wave steps. */
#define GENIE_PAIR_LANE_MAX 64
#define GENIE_PAIR_TILE 256
int64_t genie_pair_alignments_workspace_bytes(int64_t N, int64_t n_records);
int genie_pair_alignments(const genie_index *ix, int64_t N,
                          const int64_t *d_sel_offsets,     /* N + 1 */
                          const int32_t *d_records,         /* 12 * n_records, 16-byte aligned */
                          int64_t n_records,
                          const int32_t *d_class,           /* 4 * cap_chains, 16-byte aligned */
                          int64_t cap_chains,
                          int32_t orient, int32_t isize_min, int32_t isize_max, int32_t isize_mean, int32_t pen_slope,
                          int32_t pen_max, int32_t pen_unpaired, int32_t mapq_boost,
                          int32_t *d_pairs,                 /* 8 * N / 2, 16-byte aligned */
                          int32_t *d_sam,                   /* 4 * n_records, 16-byte aligned */
                          int64_t *d_totals,                /* 4, may be NULL */
                          void *d_workspace, int64_t workspace_bytes, void *stream);

/* Mate rescue, step 1: which strand-reads to seed again, and in which window of the reference.  genie_pair_alignments can only
 * choose among the records that the global seeding produced; a mate without a MEM of min_len bases has none.  Its partner, where
 * that has a record, fixes the mate's strand and places it within isize_max bases: this call writes that place down as a window
 * per strand-read, and genie_window_mems (below) seeds the window with a short minimum length.  Everything is integer and
 * deterministic.
 * Inputs:
 *   ix       for the reference length n, the device and the launch sizes.
 *   contigs  d_contig_offsets, n_contigs as genie_align_chains takes them; NULL with n_contigs == 0: one contig [0, n).
 *   reads    d_read_offsets[N + 1], used for the read lengths alone; N even (GENIE_E_INVALID otherwise), mate m of pair k is
 *            read 2 k + m as in genie_pair_alignments.
 *   records  d_sel_offsets[N + 1], d_records (12 int32 per record), n_records as genie_select_alignments wrote them;
 *            R = min(d_sel_offsets[N], n_records) as in genie_pair_alignments.  Of d_sel_offsets only entry N is used.
 *   d_pairs  8 int32 per pair, as genie_pair_alignments wrote it; columns 0 to 2 (rec0, rec1, flags) are read.
 * Parameters (int32; the call has no defaults): orient in [1, 7] with genie_pair_alignments' bits (bit 0 FR, bit 1 RF, bit 2
 * same strand); isize_max in [1, GENIE_WINDOW_MAX / 2]; min_anchor_score in [0, 2^30].
 * Units.  U = 2 N: unit 2 r + s is strand s of read r; both strands are implied, as GENIE_READS_BOTH_STRANDS numbers them.
 * Rule, per pair k and mate m (both mates may be targets):
 *   1. Mate m is a TARGET iff the pair's proper bit (flags bit 1) is clear, the other mate has a chosen record a with 0 <= a < R,
 *      and a's score (column 9) is >= min_anchor_score.  A target without bases (an empty read) gets no window.
 *   2. Of a: its strand s_a (column 3, anything but 0 taken as 1), its contig c (column 4) clamped to [0, n_contigs), b =
 *      offset - 1 (column 5), e = b + r_span (column 6), both inside the contig, and the contig's bounds [clo, chi) in the
 *      concatenation, themselves clamped to 0 <= clo <= chi <= n.
 *   3. The target's OPPOSITE-strand unit (s = 1 - s_a) gets a window iff orient has FR or RF: the hull of the allowed sides,
 *        RIGHT [b, b + isize_max)   allowed iff (FR and s_a == 0) or (RF and s_a == 1),
 *        LEFT  [e - isize_max, e)   allowed iff (FR and s_a == 1) or (RF and s_a == 0).
 *   4. The target's SAME-strand unit (s = s_a) gets [e - isize_max, b + isize_max) iff orient has bit 2.
 *   5. Both ends are clamped to [0, chi - clo], the window is cut to GENIE_WINDOW_MAX bases from its start and moved to the
 *      concatenation by + clo; an empty window is none.
 * Every other unit has no window.
 * Property.  Let y be any record of the target on the contig of a whose combination with a is concordant under
 * genie_pair_alignments' definition with the same orient and isize_max and any isize_min.  Then the reference interval [b_y, e_y)
 * of y lies inside the window of y's unit: for type FR with a the forward record, b <= b_y and e_y - b = span <= isize_max
 * (RIGHT); with a the reverse record, e_y <= e and e - b_y = span <= isize_max (LEFT); RF mirrors the two; with equal strands
 * max(e, e_y) - min(b, b_y) <= isize_max bounds both ends.  isize_max <= GENIE_WINDOW_MAX / 2, so the cut of step 5 removes
 * nothing while r_span >= 0.
 * Outputs, in caller buffers:
 *   d_windows  2 int32 per unit, 8-byte aligned: (wb, we), 0-based and half-open in the concatenation; (0, 0): no window.
 *              Written for all 2 N units.
 *   d_totals   3 int64, 8-byte aligned, may be NULL: {units with a window, pairs with at least one, reads that are targets}; it
 *              stays on the device.
 * Garbage records or pair rows give undefined windows, but no access outside the declared sizes, and every window written
 * satisfies 0 <= wb <= we <= n and we - wb <= GENIE_WINDOW_MAX.  No atomic decides a value.
 * Checked before the device check, so on any handle, in this order.  GENIE_E_INVALID: a null ix or d_sel_offsets; a negative
 * or odd N, a negative size; for N > 0 a null d_read_offsets, d_pairs or d_windows; a null d_records with n_records > 0; a
 * parameter outside its range; d_records or d_pairs not 16-byte, d_read_offsets, d_sel_offsets, d_windows or d_totals not 8-byte
 * aligned; a null table with n_contigs != 0, a table not 8-byte aligned or with n_contigs < 1 (GENIE_E_TOO_LONG for n_contigs
 * above 2^31 - 2).  Then GENIE_E_TOO_LONG for N or n_records above 2^31 - 1.  Then, for N > 0, a d_workspace that is null, not
 * 256-byte aligned or smaller than genie_rescue_windows_workspace_bytes(N) gives GENIE_E_CAPACITY.  Then GENIE_E_NO_DEVICE.  The
 * record offsets are checked on the device as genie_pair_alignments checks them (GENIE_E_INVALID), at the cost of the call's only
 * synchronisation of `stream`.  N == 0 writes zero totals and nothing else.
 * The workspace function returns GENIE_E_INVALID for a negative N, is a multiple of 256 and monotone: 256 bytes for the verdict
 * of the offset check and 4 bytes per read (the target mark), rounded up to 256.
 * Kernels: one lane per read, then one block for the totals.  Cost: three 16-byte loads per read. */
#define GENIE_WINDOW_MAX 65536       /* bases of a window: a choice (a window never spans more than two inserts), not a measurement */
int64_t genie_rescue_windows_workspace_bytes(int64_t N);
int genie_rescue_windows(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs,
                         const int64_t *d_read_offsets,    /* N + 1 */
                         int64_t N,
                         const int64_t *d_sel_offsets,     /* N + 1 */
                         const int32_t *d_records,         /* 12 * n_records, 16-byte aligned */
                         int64_t n_records,
                         const int32_t *d_pairs,           /* 8 * N / 2, 16-byte aligned */
                         int32_t orient, int32_t isize_max, int32_t min_anchor_score,
                         int32_t *d_windows,               /* 2 * 2 N, 8-byte aligned */
                         int64_t *d_totals,                /* 3, may be NULL */
                         void *d_workspace, int64_t workspace_bytes, void *stream);

/* The insert-size distribution of a paired batch, estimated from the batch itself: what genie_pair_alignments and
 * genie_rescue_windows ask their caller for (orient, isize_min, isize_max, isize_mean) and nobody knows before mapping.  The
 * pairs whose two heads map confidently to one contig are the sample, as in BWA-MEM's mem_pestat; per combination type their
 * spans give quartiles, a mean and a deviation without the outliers, and a window.  Everything is integer and deterministic.
 * Inputs, those of genie_pair_alignments:
 *   ix       used for the device and the launch sizes.
 *   N        the number of reads, even (GENIE_E_INVALID otherwise); P = N / 2; mate m of pair k is read 2 k + m.
 *   records  d_sel_offsets[N + 1], d_records (12 int32 per record) and n_records: genie_select_alignments' outputs.
 *            R = min(d_sel_offsets[N], n_records).  The records of read r are the rows [so[r], so[r + 1]) clamped to [0, R] and
 *            ordered; its HEAD is the first of them.  Of a head the columns strand, contig, offset, r_span and mapq are read.
 * Parameters (int32; the call has no defaults): min_mapq in [0, 60]; max_span in [1, GENIE_WINDOW_MAX / 2], so that an estimated
 * isize_max is always one that genie_rescue_windows accepts; min_samples in [1, 2^30].
 * Sample.  Pair k gives a sample (t, s) iff both mates have a head; both heads' mapq column, clamped to [0, 60], is >= min_mapq;
 * the heads share a contig; t, the combination type of the two heads exactly as genie_pair_alignments defines it (b = offset - 1,
 * e = b + r_span, a strand other than 0 taken as 1), is FR (0), RF (1) or same (2), type 3 gives no sample; and
 * 1 <= s <= max_span, where s = max(e) - min(b) is that definition's span.
 * Per type t, over its n_t samples in ascending order v[0 .. n_t), with integer division:
 *   q25 = v[min(n_t - 1, (n_t + 1) / 4)], q50 = v[n_t / 2], q75 = v[min(n_t - 1, (3 n_t + 1) / 4)]
 *         (BWA's (int)(p n + .499) ranks); IQR = q75 - q25;
 *   lo_b = max(1, q25 - GENIE_ISIZE_OUTLIER_IQR IQR), hi_b = q75 + GENIE_ISIZE_OUTLIER_IQR IQR: the outlier bounds;
 *   over the n_in samples with lo_b <= s <= hi_b, their sum S:
 *     mean = floor((2 S + n_in) / (2 n_in));  SS = sum of (s - mean)^2;
 *     std  = the smallest d >= 0 with d d n_in >= SS: a ceiling, in whole bases.  max_span <= 2^15 and n_in < 2^30: nothing
 *            leaves int64;
 *   isize_min = max(0, min(q25 - GENIE_ISIZE_WINDOW_IQR IQR, mean - GENIE_ISIZE_WINDOW_STD std)),
 *   isize_max = min(max_span, max(q75 + GENIE_ISIZE_WINDOW_IQR IQR, mean + GENIE_ISIZE_WINDOW_STD std)).
 * A type is OK iff n_t >= min_samples and 20 n_t >= the largest n of the three types (BWA's 5 % rule).  A type that is not OK
 * still reports n and, when n > 0, its quartiles; its other columns are 0.
 * Outputs, in caller buffers:
 *   d_stats    3 x 12 int64, 8-byte aligned, one row per type:
 *              (n, ok, q25, q50, q75, lo_b, hi_b, n_in, mean, std, isize_min, isize_max)
 *   d_samples  2 int32 per pair, 8-byte aligned, may be NULL: (t, s) of a pair with a sample, (-1, 0) of any other; for
 *              histograms and tests.
 *   d_totals   4 int64, 8-byte aligned, may be NULL: {pairs with both mates mapped, pairs sampled, pairs refused for mapq alone
 *              (contig, type and span would do), pairs refused for contig, type or span (whatever their mapq)}: the first is the
 *              sum of the other three; it stays on the device.
 * No atomic decides a value: the spans are counted into a histogram of max_span + 1 bins per type and the totals are summed with
 * atomic adds, but every such sum is an integer add, so the counts, and with them every output, do not depend on the order in
 * which the adds arrive.  Garbage records (negative r_span, wild offsets, contigs, strands, mapq) give undefined statistics, but
 * no access outside the declared sizes and no unbounded loop: the record ranges are clamped to [0, R] and ordered, a span outside
 * [1, max_span] is never counted, and every loop runs over at most max_span + 1 bins.
 * Checked before the device check, so on any handle, in this order.  GENIE_E_INVALID: a null ix, d_sel_offsets or d_stats; an
 * odd or negative N, a negative size; a null d_records with n_records > 0; a parameter outside its range; d_records not 16-byte,
 * d_sel_offsets, d_stats, d_samples or d_totals not 8-byte aligned.  Then GENIE_E_TOO_LONG for N or n_records above 2^31 - 1.
 * Then, for N > 0, a d_workspace that is null, not 256-byte aligned or smaller than
 * genie_insert_size_stats_workspace_bytes(N, max_span) gives GENIE_E_CAPACITY.  Then GENIE_E_NO_DEVICE.  The record offsets are
 * checked on the device as genie_pair_alignments checks them (GENIE_E_INVALID), at the cost of the call's only synchronisation
 * of `stream`.  N == 0 writes zero stats and zero totals and nothing else.
 * The workspace function returns GENIE_E_INVALID for a negative N or a max_span outside its range, is a multiple of 256 and
 * monotone in both: 256 bytes for the verdict of the offset check, 256 for the four totals, and 12 bytes per bin (a 4-byte
 * counter for each of the three types) for max_span + 1 bins, rounded up to 256; nothing per pair.
 * Kernels: one lane per pair reads three offsets and the three 16-byte rows of each head, writes d_samples and counts the span:
 * spans below GENIE_ISIZE_LDS_BINS in a histogram of the block in LDS, whose non-zero bins the block adds to the global one when
 * it is done, spans from GENIE_ISIZE_LDS_BINS on in the global one at once; the totals are summed over the block and added once.
 * Then one block, 256 lanes per type, finds the three ranks by a scan over the bins, passes over [lo_b, hi_b] for n_in and S
 * and again for SS, bisects std over [0, max_span] and writes the 36 numbers.  Nothing is sorted. */
#define GENIE_ISIZE_OUTLIER_IQR 2    /* the three multipliers are BWA-MEM's: choices, not measurements */
#define GENIE_ISIZE_WINDOW_IQR 3
#define GENIE_ISIZE_WINDOW_STD 4
#define GENIE_ISIZE_LDS_BINS 4096    /* spans counted in LDS: a choice sized to three 48 KB blocks on a compute unit */
int64_t genie_insert_size_stats_workspace_bytes(int64_t N, int32_t max_span);
int genie_insert_size_stats(const genie_index *ix, int64_t N,
                            const int64_t *d_sel_offsets,   /* N + 1 */
                            const int32_t *d_records,       /* 12 * n_records, 16-byte aligned */
                            int64_t n_records,
                            int32_t min_mapq, int32_t max_span, int32_t min_samples,
                            int64_t *d_stats,               /* 3 * 12 */
                            int32_t *d_samples,             /* 2 * N / 2, 8-byte aligned, may be NULL */
                            int64_t *d_totals,              /* 4, may be NULL */
                            void *d_workspace, int64_t workspace_bytes, void *stream);

/* Mate rescue, step 2, and a general call: the MEMs of strand-reads against WINDOWS of the reference, added to the MEM rows of
 * the batch.  Any windows will do, not only genie_rescue_windows'.  The index is not consulted: a window is compared with the
 * strand-read base for base, so a min_len that would be meaningless against the whole reference (12, say) costs the window's
 * size and not the number of its occurrences in the genome.  The rows that come out are ordinary MEM rows: genie_chain_mems and
 * everything behind it run on them unchanged.
 * Inputs:
 *   ix       for the packed reference and its length n.
 *   reads    flags, d_bases, d_read_offsets, N, total_bases, max_len exactly as genie_align_chains takes them:
 *            GENIE_READS_BOTH_STRANDS gives S = 2 (else 1) with unit u = S i + s read i on strand s, strand 1 the reverse
 *            complement, built on the fly; GENIE_READS_SPLIT_BREAKS is accepted and changes nothing.  U must equal S N.
 *   windows  d_windows: 2 int32 per unit, (wb, we), 0-based and half-open.  The call clamps both ends to [0, n]; we <= wb after
 *            that is an empty window (so is we < wb before it); then we is cut to wb + GENIE_WINDOW_MAX.
 *   min_len  m >= 1.
 *   input rows (optional)  d_in_offsets[U + 1], d_in_rows (4 int32 per row), in_total_rows: rows as genie_find_mems* wrote them.
 *            d_in_offsets == NULL: no unit has input rows.  The offsets are checked on the device as genie_chain_mems checks
 *            its row offsets (first 0, non-decreasing, last <= in_total_rows, no unit above 2^31 - 1 rows).
 * Window rows of unit u.  Q is the strand-read, L its length, [wb, we) its window.  A window row is every (p, t, l) with
 *   l >= m, wb <= t and t + l <= we;
 *   Q[p .. p+l) == T[t .. t+l) base for base, every query code <= 3 (a code > 3 differs from everything);
 *   left-maximal INSIDE THE WINDOW   p == 0, or t == wb, or Q[p-1] != T[t-1];
 *   right-maximal                    p + l == L, or t + l == we, or Q[p+l] != T[t+l]:
 * the MEMs of Q against T[wb .. we) taken as a reference of its own.  The row is (p, p + l, t + 1, -1): no suffix-array row is
 * looked up.  A MEM of the whole reference that reaches beyond the window appears clipped to it.
 * Output of a unit.  Without a window: its input rows, byte for byte and in their order.  With a window: the set union of its
 * input rows and its window rows on the triple (start, end, pos), sorted ascending by (start, pos, end), all three as signed
 * integers; column 3 is that of the first input row that has the triple, else -1.  The start order is what genie_chain_mems
 * needs; the rest makes the output a function of the inputs alone.
 * Caps, which bound the work and are no policy.  d_status[u] is 0 for a unit without a window and else exactly one of
 *   1  searched: the unit's output is the union above;
 *   2  its input rows plus its window rows, counted before the union, exceed GENIE_WINDOW_MAX_ROWS: it keeps its input rows
 *      as they are;
 *   4  L > GENIE_MAX_READ_LEN: it keeps its input rows as they are.
 * GENIE_WINDOW_MAX and GENIE_WINDOW_MAX_ROWS are choices sized to LDS (the rows of a unit are ranked in a 32 KB table of one
 * wave), not measurements.
 * Outputs, all in caller buffers:
 *   d_offsets  U + 1 int64, 8-byte aligned; [U] holds the true total even past out_cap_rows
 *   d_rows     4 int32 per row, 16-byte aligned, out_cap_rows of them; NULL is the sizing call (offsets, status and totals are
 *              written all the same).  Rows past the capacity are dropped.
 *   d_status   U int32, may be NULL
 *   d_totals   3 int64, 8-byte aligned, may be NULL: {rows in all, window rows added after the union, units over a cap}
 * Memory-safe on any windows and any input rows: the loops are bounded by L, the window length and the row cap, and rows that
 * break genie_find_mems' form come out with undefined order but inside the declared sizes.  One integer atomicAdd in LDS hands
 * out the places of the rows found in a wave's table; it decides no value, since those rows are distinct and the output order
 * is the rank of the keys.
 * Checked before the device check, so on any handle, in this order.  GENIE_E_INVALID: a null ix, d_offsets or d_read_offsets, a
 * null d_bases (total_bases > 0), a negative N, total_bases or max_len, max_len above 2^31 - 1, an unknown flag bit; a negative
 * U, out_cap_rows, in_total_rows or workspace_bytes, U != S N, min_len < 1; a null d_windows with U > 0, a null d_in_rows with
 * d_in_offsets and in_total_rows > 0; d_rows or d_in_rows not 16-byte, d_offsets, d_in_offsets, d_read_offsets, d_windows or
 * d_totals not 8-byte, d_status not 4-byte aligned.  Then GENIE_E_TOO_LONG for U above 2^31 - 1.  Then, for U > 0, a
 * d_workspace that is null, not 256-byte aligned or smaller than genie_window_mems_workspace_bytes(U) gives GENIE_E_CAPACITY.
 * Then GENIE_E_NO_DEVICE.  Bad read offsets or input row offsets give GENIE_E_INVALID, found on the device at the cost of the
 * call's only synchronisation of `stream`.  U == 0 writes d_offsets[0] = 0 and zero totals.
 * The workspace function returns GENIE_E_INVALID for a negative U, is a multiple of 256 and monotone: 56 bytes per unit (its
 * clamped window 8, the search mark 4, its row count 4, its new rows 4, its status 4, its row in the list of units to search
 * twice 16), that list's offsets 8 (U + 1) and 8 per 1024 units (the scan), each piece rounded up to 256 on its own, and 256 for
 * the verdict of the offset checks; nothing per row.
 * Kernels: the units with a window are compacted into a list and run one wave each (blocks of one wave: 37 KB of LDS, four
 * to a CU).  The wave packs the strand-read to 2 bits a base in LDS, with the mask of its codes > 3, and takes the L + B - 1
 * diagonals d = t - p of a window of B bases 64 at a time; a lane walks its diagonal in 32-base words, the XOR of the query
 * word with the reference word folded to a bit per base, the runs taken by bit scans.  The rows are ranked by counting the
 * smaller keys in LDS.  Count, scan, fill: the walk runs twice.  Cost of a unit: about ceil((L + B - 1) / 64) ceil(L / 32) wave
 * steps a pass, and K^2 / 64 for the rank of its K rows. */
#define GENIE_WINDOW_MAX_ROWS 2048
int64_t genie_window_mems_workspace_bytes(int64_t U);
int genie_window_mems(const genie_index *ix, int32_t flags, const uint8_t *d_bases, const int64_t *d_read_offsets,
                      int64_t N, int64_t total_bases, int64_t max_len,
                      int64_t U,
                      const int32_t *d_windows,        /* 2 * U, 8-byte aligned */
                      int32_t min_len,
                      const int64_t *d_in_offsets,     /* U + 1, may be NULL: no input rows */
                      const int32_t *d_in_rows,        /* 4 * in_total_rows, 16-byte aligned */
                      int64_t in_total_rows,
                      int64_t *d_offsets,              /* U + 1 */
                      int32_t *d_rows,                 /* 4 * out_cap_rows, 16-byte aligned; may be NULL: counting only */
                      int64_t out_cap_rows,
                      int32_t *d_status,               /* U, may be NULL */
                      int64_t *d_totals,               /* 3, may be NULL */
                      void *d_workspace, int64_t workspace_bytes, void *stream);

/* The SAM records of a mapped batch as TEXT in device memory: the output end of the pipeline.  One line per record, read by read
 * and for each read its records in record order; a read without records gets one unmapped line.  Every line ends with '\n'.
 * Inputs, all on the device:
 *   ix       for the packed reference (the letters of MD) and its length n.
 *   table    d_contig_offsets and n_contigs as the *_contigs calls take them; NULL and 0: one contig that starts at position 0.
 *            Only the start of a record's contig is read, clamped to [0, n]; nc = max(n_contigs, 1) contig names exist.
 *   reads    d_bases (codes 0..4, read orientation), d_read_offsets[N + 1], total_bases; d_quals, which may be NULL, holds
 *            total_bases bytes under the same offsets.
 *   records  d_sel_offsets[N + 1], d_records (12 int32 per record) and n_records as genie_select_alignments wrote them;
 *            R = min(d_sel_offsets[N], n_records), and the records of read r are the rows [so[r], so[r + 1]) cut to [0, R), as
 *            in genie_pair_alignments.  d_sam (4 int32 per record: flag, mapq, mate_record, tlen), genie_pair_alignments'; NULL
 *            is SINGLE-END mode.  d_info (8 int32 per record), d_cigar_offsets[R + 1] and d_cigar (n_ops ops, length << 4 |
 *            code, codes 1 I, 2 D, 4 S, 7 =, 8 X) as genie_chain_cigars wrote them for these records.
 *   names    d_names and d_name_offsets[N + 1] (name_bytes bytes), one name per read; d_contig_names and
 *            d_contig_name_offsets[nc + 1] (contig_name_bytes bytes).
 *   tags     a mask of GENIE_SAM_NM (1), _AS (2), _MD (4), _MC (8), _MQ (16); the tags are written in that order.
 *   flags    GENIE_SAM_NO_SEQ: SEQ and QUAL are `*`.
 * With d_sam, N is even and reads 2 k and 2 k + 1 are mates.
 * A record line (record j of read r): QNAME the read's name; FLAG and MAPQ d_sam's; RNAME the name of the record's contig
 * (its index clamped to [0, nc)); POS its offset column; CIGAR the text of its ops, `*` for none; with m = d_sam's mate_record
 * (none unless 0 <= m < R) RNEXT is `*` and PNEXT 0 for none, else RNEXT is `=` when record m has the same contig column and
 * its contig's name otherwise, and PNEXT its offset; TLEN d_sam's; SEQ from the codes, 0..3 A C G T and anything else N, and
 * QUAL the bytes of d_quals (`*` with d_quals == NULL): for a record whose strand column is not 0 SEQ is the complement written
 * in reverse (N stays N) and QUAL reversed; a read of no bases has an empty SEQ.  Numbers are signed decimals.  Then the tags,
 * each behind a tab: NM:i: (d_info column 3), AS:i: (the score column), MD:Z: only for a record that has ops, MC:Z: and MQ:i:.
 * The unmapped line of read r: m is the LAST record in the range of read r ^ 1 whose d_sam flag has neither 0x100 nor 0x800;
 * FLAG is 0x1 | 0x4 | (0x40 for an even r, 0x80 for an odd one) | (0x8 without m) | (0x20 when m's strand is not 0); with m RNAME
 * and POS are m's, RNEXT is `=` and PNEXT is POS, else `*`, 0, `*`, 0; MAPQ 0, CIGAR `*`, TLEN 0; SEQ and QUAL in read
 * orientation; of the tags only MC and MQ.
 * MC is the CIGAR text of record m, written when m exists and has ops; MQ is d_sam's mapq of record m, written when m exists.
 * MD is a function of the CIGAR and the reference alone.  t = the contig's start + POS - 1, c = 0 (an int64); an = of length L:
 * c += L, t += L; an X of length L: for each base write c and the reference letter at t, then c = 0 and t += 1; a D of length
 * L: write c, `^` and the L reference letters from t on, then c = 0 and t += L; I and S: nothing; at the end write c.  Examples:
 * 5A0C3, 0A7, 4^AC0T2.  A reference position outside [0, n) is clamped: an undefined letter.
 * Single-end mode (d_sam == NULL): N need not be even; FLAG = 0x10 (strand) | 0x800 (kind 1) | 0x100 (kind 2), MAPQ the record's
 * mapq column, RNEXT `*`, PNEXT 0, TLEN 0; the unmapped line has FLAG 4 and `* 0 0 * * 0 0`; MC and MQ are never written.
 * Outputs, all in caller buffers:
 *   d_line_offsets  N + n_records + 1 int64 of capacity, 8-byte aligned; with n_lines = R + (reads without records) the entries
 *                   0 .. n_lines are written, entry [n_lines] the true byte total even when cap_text is smaller
 *   d_text          cap_text bytes; NULL is the sizing call.  Line l is the bytes [d_line_offsets[l], d_line_offsets[l + 1]);
 *                   bytes at or past cap_text are dropped and nothing is written outside the buffer
 *   d_totals        3 int64, 8-byte aligned, may be NULL: {lines, bytes, unmapped lines}; it stays on the device
 * No atomic decides a value: the text is a function of the inputs alone.  Garbage records, d_sam or d_info rows or ops give
 * undefined bytes, but no access outside the declared sizes and no unbounded loop: record ranges, record, contig and reference
 * indices are clamped, every store lies below min(the line's end, cap_text), and the loop over the letters of an X or a D ends
 * there too.  A line of more than 2^31 - 1 bytes is cut to that length.
 * Checked before the device check, so on any handle, in this order.  GENIE_E_INVALID: a null ix, d_read_offsets, d_sel_offsets,
 * d_name_offsets, d_contig_name_offsets or d_line_offsets; a negative size; an odd N with d_sam; an unknown bit in tags or
 * flags; a null d_bases, d_names, d_contig_names or d_cigar whose size is above 0; a null d_records, d_info or d_cigar_offsets
 * with n_records > 0; d_records, d_sam or d_info not 16-byte, an offset array, d_line_offsets or d_totals not 8-byte, d_cigar not
 * 4-byte aligned; a null table with n_contigs != 0, a table with n_contigs < 1 or not 8-byte aligned.  Then GENIE_E_TOO_LONG for
 * n_contigs, N or n_records above 2^31 - 1.  Then, for N > 0, a d_workspace that is null, not 256-byte aligned or smaller than
 * genie_sam_text_workspace_bytes(N, n_records) gives GENIE_E_CAPACITY.  Then GENIE_E_NO_DEVICE.  The five offset arrays are
 * checked on the device as genie_chain_mems checks its row offsets (first 0, non-decreasing, last at most the array's declared
 * total -- d_sel_offsets has none --, no item above 2^31 - 1; d_cigar_offsets over its first R + 1 entries): GENIE_E_INVALID, at
 * the cost of the call's only synchronisation of `stream`.  N == 0 writes d_line_offsets[0] = 0 and zero totals.
 * The workspace function returns GENIE_E_INVALID for negative arguments, is a multiple of 256 and monotone in both: per read 4
 * (the mark of a read without records) and 8 (the number of such reads before it, N + 1 entries), per line of the N + n_records
 * there can be 8 (its read and record), 4 (its length) and 8 (its offset, one entry more), 8 per 1024 lines (the scan), each
 * piece rounded up to 256 on its own, and 256 for the verdict of the offset checks.
 * Kernels: one wave per line, in a sizing pass and a write pass over the same walk.  The lanes go over the bytes of the name, of
 * SEQ and QUAL and over the ops, 64 at a time; an op's place in CIGAR, MC and MD is a wave prefix sum over the ops' text lengths,
 * MD's count in front of an X or a D a segmented sum of the = lengths (a prefix sum less a prefix maximum).  The sizing pass loads
 * records and ops only.  Cost of a line: about (name + 2 bases) / 64 + 3 ceil(ops / 64) wave steps. */
#define GENIE_SAM_NM 1
#define GENIE_SAM_AS 2
#define GENIE_SAM_MD 4
#define GENIE_SAM_MC 8
#define GENIE_SAM_MQ 16
#define GENIE_SAM_NO_SEQ 1
int64_t genie_sam_text_workspace_bytes(int64_t N, int64_t n_records);
int genie_sam_text(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs,
                   const uint8_t *d_bases, const int64_t *d_read_offsets,  /* N + 1 */
                   int64_t N, int64_t total_bases,
                   const uint8_t *d_quals,              /* total_bases, may be NULL */
                   const int64_t *d_sel_offsets,        /* N + 1 */
                   const int32_t *d_records,            /* 12 * n_records, 16-byte aligned */
                   int64_t n_records,
                   const int32_t *d_sam,                /* 4 * n_records, 16-byte aligned; NULL: single-end mode */
                   const int32_t *d_info,               /* 8 * n_records, 16-byte aligned */
                   const int64_t *d_cigar_offsets,      /* R + 1 */
                   const uint32_t *d_cigar, int64_t n_ops,
                   const uint8_t *d_names, const int64_t *d_name_offsets /* N + 1 */, int64_t name_bytes,
                   const uint8_t *d_contig_names, const int64_t *d_contig_name_offsets /* max(n_contigs, 1) + 1 */,
                   int64_t contig_name_bytes,
                   int32_t tags, int32_t flags,
                   int64_t *d_line_offsets,             /* N + n_records + 1 */
                   uint8_t *d_text,                     /* cap_text; may be NULL: sizing only */
                   int64_t cap_text,
                   int64_t *d_totals,                   /* 3, may be NULL */
                   void *d_workspace, int64_t workspace_bytes, void *stream);

/* The same batch as uncompressed BAM ALIGNMENT RECORDS in device memory (SAMv1 section 4.2): what a BAM file holds between its
 * header and its end, before BGZF compression.  The inputs, through `tags, flags`, are genie_sam_text's in its order and with
 * its meaning, single-end mode (d_sam == NULL) included.  One record per line of genie_sam_text, in the same order: read by read
 * and for each read record by record, a read without records one unmapped record.  The record of line l has the FLAG, MAPQ,
 * contig, POS, mate record m, PNEXT, TLEN and strand that genie_sam_text derives for that line (above): the unmapped line's flag
 * bits, its place at the LAST record of its mate that is neither secondary nor supplementary, and the single-end rules are
 * those and are not restated here.
 * The bytes of a record, little-endian, no padding; records lie back to back, so a record starts at any byte alignment:
 *   block_size  int32   the record's length minus 4
 *   refID       int32   RNAME's contig index clamped to [0, nc), -1 where the line has `*`
 *   pos         int32   POS - 1
 *   l_read_name uint8   the stored name's length + 1
 *   mapq        uint8   MAPQ clamped to [0, 255]
 *   bin         uint16  SAMv1's reg2bin(beg, end) on int64 with arithmetic shifts, cut to 16 bits: beg = pos, end = beg + the
 *                       sum of the lengths of the ops with the codes 0, 2, 3, 7, 8, or beg + 1 when that sum is 0; pos -1
 *                       gives 4680
 *   n_cigar_op  uint16
 *   flag        uint16  FLAG's low 16 bits
 *   l_seq       int32   the read's length, 0 under GENIE_SAM_NO_SEQ
 *   next_refID  int32   -1 for RNEXT `*`, else record m's contig index clamped (for `=` that is refID)
 *   next_pos    int32   PNEXT - 1
 *   tlen        int32
 *   read_name   the name's first min(length, 254) bytes and a NUL; an empty name is stored as `*`
 *   cigar       the record's ops as they are, uint32 each; none for a record without ops
 *   seq         (l_seq + 1) / 2 bytes, base 2 i in the high nibble of byte i; codes 0..3 are 1, 2, 4, 8, anything else 15; the
 *               unused low nibble of an odd length is 0.  A record whose strand column is not 0 has the complement in reverse
 *               order (N stays N), as SEQ in genie_sam_text
 *   qual        l_seq bytes max(q - 33, 0), reversed on that strand; every byte 0xFF with d_quals == NULL
 *   tags        NM, AS, MD, MC, MQ in that order under the text's conditions: NM and AS on record lines only, MD on a record
 *               with ops, MC when m exists and has ops, MQ when m exists; an unmapped record has MC and MQ only.  NM, AS, MQ
 *               are of type `i` (two letters, `i`, int32: 7 bytes); MD and MC of type `Z`: two letters, `Z`, the characters
 *               genie_sam_text writes behind MD:Z: and MC:Z:, and a NUL
 * More than 65535 ops (SAMv1 4.2.2): n_cigar_op is 2, the cigar field holds l_seq << 4 | 4 and then min(reference span,
 * 2^28 - 1) << 4 | 3, and the real ops follow all other tags as `CG`, `B`, `I`, an int32 count and the ops; bin is still that of
 * the real ops.
 * Outputs, all in caller buffers:
 *   d_record_offsets  N + n_records + 1 int64 of capacity, 8-byte aligned; with n = R + (reads without records) the entries
 *                     0 .. n are written, entry [n] the true byte total even when cap_data is smaller
 *   d_data            cap_data bytes; NULL is the sizing call.  Record l is the bytes [d_record_offsets[l],
 *                     d_record_offsets[l + 1]); bytes at or past cap_data are dropped and nothing is written outside the buffer
 *   d_totals          3 int64, 8-byte aligned, may be NULL: {records, bytes, unmapped records}; it stays on the device
 * No atomic decides a value: the bytes are a function of the inputs alone.  Garbage records, d_sam or d_info rows or ops give
 * undefined bytes, but no access outside the declared sizes and no unbounded loop, under genie_sam_text's clamps: every store
 * lies below min(the record's end, cap_data), and the loop over the letters of an X or a D in MD ends there too.  A record of
 * more than 2^31 - 1 bytes is cut to that length, and block_size says the length it was cut to.
 * The argument checks, their order and their results are genie_sam_text's word for word, with d_record_offsets, d_data and
 * cap_data in the places of d_line_offsets, d_text and cap_text and genie_bam_records_workspace_bytes as the bound of the
 * workspace; then GENIE_E_NO_DEVICE; then the same device check of the five offset arrays, GENIE_E_INVALID, at the cost of the
 * call's only synchronisation of `stream`.  N == 0 writes d_record_offsets[0] = 0 and zero totals.
 * The workspace function returns GENIE_E_INVALID for negative arguments, is a multiple of 256 and monotone in both.  Its pieces
 * are those of genie_sam_text_workspace_bytes: per read 4 (the mark of a read without records) and 8 (the number of such reads
 * before it, N + 1 entries), per record of the N + n_records there can be 8 (its read and record), 4 (its length) and 8 (its
 * offset, one entry more), 8 per 1024 records (the scan), each piece rounded up to 256 on its own, and 256 for the verdict of
 * the offset checks.
 * Kernels: one wave per record, in a sizing pass and a write pass over the same walk.  Where a field lies is closed-form but for
 * MD and MC, so the sizing pass loads ops only when one of the two is asked for.  Nothing is stored wider than a byte, the lanes
 * of a step on consecutive addresses: one lane per byte of the name, of QUAL and of the ops, one lane per byte (two bases) of
 * SEQ; the loop that copies the ops also sums their reference span for bin, so the 36-byte head goes last.  Cost of a record:
 * about (name + 1.5 bases) / 64 + 5 ceil(ops / 64) wave steps, plus genie_sam_text's 2 ceil(ops / 64) each for MD and MC. */
int64_t genie_bam_records_workspace_bytes(int64_t N, int64_t n_records);
int genie_bam_records(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs,
                      const uint8_t *d_bases, const int64_t *d_read_offsets,  /* N + 1 */
                      int64_t N, int64_t total_bases,
                      const uint8_t *d_quals,              /* total_bases, may be NULL */
                      const int64_t *d_sel_offsets,        /* N + 1 */
                      const int32_t *d_records,            /* 12 * n_records, 16-byte aligned */
                      int64_t n_records,
                      const int32_t *d_sam,                /* 4 * n_records, 16-byte aligned; NULL: single-end mode */
                      const int32_t *d_info,               /* 8 * n_records, 16-byte aligned */
                      const int64_t *d_cigar_offsets,      /* R + 1 */
                      const uint32_t *d_cigar, int64_t n_ops,
                      const uint8_t *d_names, const int64_t *d_name_offsets /* N + 1 */, int64_t name_bytes,
                      const uint8_t *d_contig_names, const int64_t *d_contig_name_offsets /* max(n_contigs, 1) + 1 */,
                      int64_t contig_name_bytes,
                      int32_t tags, int32_t flags,
                      int64_t *d_record_offsets,           /* N + n_records + 1 */
                      uint8_t *d_data,                     /* cap_data; may be NULL: sizing only */
                      int64_t cap_data,
                      int64_t *d_totals,                   /* 3, may be NULL: {records, bytes, unmapped records} */
                      void *d_workspace, int64_t workspace_bytes, void *stream);

/* Matching statistics and SMEMs that are EXACT WITH RESPECT TO THE SEQUENCE SET.  genie_match_stats and the SMEM calls on a
 * reference of several sequences answer for the concatenation; genie_locate_contigs then drops the occurrences that bridge
 * two sequences, and with them seeds.  Contigs ACGT | TTGA and the read CGTT: the concatenation holds CGTT once, across the
 * boundary; the only SMEM is (0, 4), its only occurrence is dropped, the read has no hit.  Against the set the read has the
 * SMEMs (0, 3) (CGT in contig 0) and (2, 4) (TT in contig 1).  These two calls give the second answer.
 * Arguments: those of genie_match_stats / genie_find_smems_long_ex with the table (above) behind ix and d_totals behind
 * d_status.  Reads, flags, strand-reads, virtual positions, breaks, the offset check and the statuses are the parents'.
 * Definition.  ms_c[v], the contig-exact matching statistic, is the largest l >= 0 for which the l bases of the strand-read
 * from p on hold no break and equal T[t .. t+l) for some t with l <= room(t): they occur inside one contig.  Equivalently
 * the maximum over the contigs of the matching statistic against that contig alone.  Four facts:
 *   1  ms_c[v] <= ms[v], and ms_c[v] >= 1 iff ms[v] >= 1, because an occurrence t < n has room(t) >= 1: GENIE_READ_ABSENT_BASE
 *      and GENIE_READ_BAD_BASE are flagged exactly as by the parents.
 *   2  ms_c[v+1] >= ms_c[v] - 1 inside a strand-read, so fwd_c[p] = p + ms_c[p] is non-decreasing: the BWA traversal applies
 *      unchanged and yields the SMEMs with respect to the sequence set.
 *   3  Let p0 be a run start of the concatenation's fwd[] (p0 = 0 or fwd[p0] != fwd[p0-1]).  If some occurrence t of
 *      Q[p0 .. fwd[p0]) has room(t) >= fwd[p0] - p0, then ms_c = ms at every position of the run (occurrence t + k serves
 *      position p0 + k): only run starts need an interval and a room test, a handful per 150-base read.
 *   4  If no occurrence of the run start qualifies, the positions of the run are resolved one by one: "some t in the
 *      interval of Q[p .. p+l) has room(t) >= l" is monotone in l, so ms_c[p] is the largest l in [largest room seen, ms[p])
 *      for which it holds, found by bisection over l.
 * genie_match_stats_contigs writes d_ms[v] = ms_c[v] and, unless d_lohi is NULL, d_lohi[v] = the inclusive interval IN THE
 * CONCATENATION of those ms_c[v] bases, what genie_sa_interval returns for them: it may still hold bridging rows, at least
 * one of its rows does not bridge, genie_locate_contigs drops the others; (-1, -1) where ms_c = 0.  Bad-base strand-reads
 * get -1 and (-1, -1) as in the parent.
 * genie_find_smems_contigs writes the rows (start, end, lo, hi) that the BWA traversal produces from fwd_c, min_len and mode
 * as genie_find_smems_long_ex takes them (GENIE_READS_SPLIT_BREAKS needs GENIE_MODE_BWA); (lo, hi) is the interval of
 * Q[start .. end) in the concatenation.  Row order, d_offsets, out_cap_rows, the sizing behaviour and the unit passes are
 * the parent's.  Every row has at least one hit in genie_locate_contigs.
 *   d_totals   (1 int64, 8-byte aligned, may be NULL) the number of virtual positions with ms_c < ms: the positions that were
 *              clipped (genie_find_smems_contigs: those of the strand-reads that are not flagged, the only ones with rows).
 *              It stays on the device; no synchronisation is added for it.
 * With n_contigs == 1 both calls give the outputs of genie_match_stats and genie_find_smems_long_ex byte for byte.
 * Against genie_find_mems_contigs (same flags, min_len m): no row is longer than ms_c at its start, and at a run start of
 * fwd_c (p == 0 or fwd_c[p] != fwd_c[p-1]) with ms_c >= m the longest row that starts there is ms_c long.  At other
 * positions the longest contig-exact match can be extended to the left and need not be a row: MEMs are left-maximal.
 * Checks, all before the device check: the parent's, in its order (GENIE_E_INVALID; an unknown flag bit included), then a
 * misaligned d_totals and the table's (GENIE_E_INVALID, GENIE_E_TOO_LONG for n_contigs above 2^31 - 2), then for N > 0 a
 * workspace that is null, not 256-byte aligned or smaller than the size function's value (GENIE_E_CAPACITY), then
 * GENIE_E_NO_DEVICE on a host-only handle.  The table is NOT validated; the calls are memory-safe on any table contents.
 * The workspace functions return GENIE_E_INVALID for what the call refuses, are multiples of 256, monotone in every argument
 * and at least the parent's size for the same batch: the parent's plus 8 S bytes per base (the slow list's slots), 6 per
 * window of 256 positions and per unit (the flagged run starts per window and per four windows) and 8 KB (clip counts).  The parent's part is
 * used at its declared size: a larger workspace does not widen the unit passes.
 * Kernels: the parent's pack and forward stages give fwd[] of the concatenation; one kernel tests every run start (its
 * interval, then SaRec.s of its rows with early exit, one lane up to 32 rows and the whole wave beyond, room through the
 * staged table) and appends the failing ones to a slow list placed by window counts and a scan; a second, rare, kernel
 * resolves the positions of those runs by fact 4 and rewrites their fwd[]; then the parent's statistics kernel, or a small
 * kernel that rebuilds the window maxima and marks followed by the parent's traversal, run over the corrected fwd[].  No
 * atomic decides a value.  Synchronisations of `stream`: the parents' and no more.
 * Cost: the parent's plus, per run start, one interval and its rows up to the first that has room; a flagged run costs per
 * position a few interval searches (one at ms, a gallop up from the largest room seen, at most log2(ms) more), each
 * followed by a walk of that interval's rows -- all of them where none has room, so a reference of very many very short contigs under long matches is the expensive case. */
int64_t genie_match_stats_contigs_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags, int64_t n_contigs);
int genie_match_stats_contigs(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t flags,
                              const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N, int64_t total_bases,
                              int64_t max_len,
                              int32_t *d_ms,           /* S * total_bases */
                              int32_t *d_lohi,         /* 2 * S * total_bases, may be NULL */
                              int32_t *d_status,       /* S * N, may be NULL */
                              int64_t *d_totals,       /* 1, may be NULL: positions clipped */
                              void *d_workspace, int64_t workspace_bytes, void *stream);
int64_t genie_find_smems_contigs_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags, int64_t n_contigs);
int genie_find_smems_contigs(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t mode,
                             int32_t flags, const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N,
                             int64_t total_bases, int64_t max_len, int32_t min_len,
                             int64_t *d_offsets,      /* S * N + 1 */
                             int32_t *d_rows,         /* 4 * out_cap_rows, 16-byte aligned */
                             int64_t out_cap_rows,
                             int32_t *d_status,       /* S * N, may be NULL */
                             int64_t *d_totals,       /* 1, may be NULL: positions clipped */
                             void *d_workspace, int64_t workspace_bytes, void *stream);

/* Matching statistics and SMEMs under a MINIMUM OCCURRENCE COUNT: the longest match that occurs at least k = min_occ times in
 * the reference (BWA-MEM's min_intv).  Every other seeding call answers "the longest match" whatever its number of
 * occurrences; a read inside one copy of a diverged repeat then gets one seed and never sees the other copies.  Re-seeding is
 * the caller's loop over this call: a long SMEM of occ occurrences is asked again with k = occ + 1 (k = 2 .. split_width + 1
 * in BWA-MEM's terms), and the rows that cover the SMEM's midpoint are kept.  No policy is built in; k is one scalar.
 * Arguments: those of genie_match_stats / genie_find_smems_long_ex with min_occ behind flags / min_len and d_totals behind
 * d_status.  Reads (CSR, any length), flags, strand-reads, virtual positions v, the offset check and the synchronisations
 * are the parents'.
 * Definition.  occ(w) is the number of suffix-array rows whose suffix starts with w (the $ row never counts; hi - lo + 1 of
 * genie_sa_interval for an occurring w).  ms_k[v] is the largest l >= 0 for which the l bases of the strand-read from p on
 * hold no break and occur at least k times.  ms_1 = ms.  fwd_k[p] = p + ms_k[p].  Five facts:
 *   1  ms_k <= ms, and ms_k is non-increasing in k.  ms_k[p] = 0 iff the base at p is a break or occurs fewer than k times in
 *      the reference: a base RARE AT K ("the reference lacks it" is k = 1).
 *   2  ms_k[v+1] >= ms_k[v] - 1 inside a strand-read (dropping the first base can only gain occurrences), so fwd_k is
 *      non-decreasing; "Q[s..e) occurs >= k times" <=> fwd_k[s] >= e, because occ is monotone in the length.  So the BWA
 *      traversal applied to fwd_k yields exactly the matches of >= k occurrences that no other such match contains: the
 *      SMEMs under min_intv = k.
 *   3  Let p0 be a run start of the parent's fwd[].  If the interval of Q[p0 .. fwd[p0]) has >= k rows, ms_k = ms on the
 *      whole run: every position's match is a suffix of that string.  (The same holds from any position to the run's end.)
 *   4  Otherwise each position is resolved on its own: occ(Q[p..p+l)) >= k is monotone in l, bisection over [0, ms[p]].
 *   5  Without a search over l: with [lo, hi] the interval of the full match, hi - lo + 1 < k, and R = n + 1 rows,
 *      ms_k[p] = max over a in [max(1, hi-k+1), min(lo, R-k)] of min(ms[p], lcp(T[SA[a]..], T[SA[a+k-1]..])), 0 when the
 *      range is empty.  Equivalently the k-th largest of L_j = min(ms[p], lcp(Q[p..], T[SA[j]..])) over the rows j >= 1,
 *      which is how the kernel takes it: rows from either side of [lo, hi], the larger L_j first, until k are together.
 * Status and breaks.  Without GENIE_READS_SPLIT_BREAKS a strand-read that holds a base rare at k is flagged
 * GENIE_READ_ABSENT_BASE and has no SMEM rows; its statistics are written and correct all the same.  GENIE_READ_BAD_BASE is
 * the parent's.  With GENIE_READS_SPLIT_BREAKS a base rare at k is a break and every status is GENIE_READ_OK.  The four base
 * counts are taken from the prefix directory on the device.
 * genie_match_stats_min_occ writes d_ms[v] = ms_k[v] and, unless d_lohi is NULL, d_lohi[v] = the interval of those ms_k
 * bases -- at least k rows wherever ms_k > 0, (-1, -1) where ms_k = 0.  Bad-base strand-reads get -1 and (-1, -1).
 * genie_find_smems_min_occ writes the rows (start, end, lo, hi) the traversal produces from fwd_k, hi - lo + 1 >= k on every
 * row; mode, min_len, row order, d_offsets, out_cap_rows, the sizing behaviour and the unit passes are the parent's
 * (GENIE_READS_SPLIT_BREAKS needs GENIE_MODE_BWA).
 *   d_totals   (1 int64, 8-byte aligned, may be NULL) the number of virtual positions with ms_k < ms
 *              (genie_find_smems_min_occ: those of the strand-reads that are not flagged), ms taken under the call's own
 *              breaks: with GENIE_READS_SPLIT_BREAKS a base rare at k ends the match of either.  It stays on the device.
 * With min_occ == 1 both calls give the outputs of genie_match_stats / genie_find_smems_long_ex byte for byte.  With
 * GENIE_READS_BOTH_STRANDS they give those of the call without the flag on the explicit interleaved batch.  No atomic
 * decides a value; nothing outside the declared sizes is written.
 * Checks, all before the device check: the parent's, in its order; then min_occ < 1 and a misaligned d_totals
 * (GENIE_E_INVALID); then the workspace (GENIE_E_CAPACITY); then GENIE_E_NO_DEVICE on a host-only handle.
 * The workspace functions take the parent's arguments, do not depend on k, return GENIE_E_INVALID for what the call refuses,
 * are multiples of 256, monotone in every argument and at least the parent's value: the parent's plus 4 bytes per window
 * of 256 positions and per unit and 8 bytes per 256 units.  The parent's part is used at its declared size.
 * Not offered: a threshold per read or per position, re-seeding itself, min_occ together with a contig table, the padded
 * and the packed host-link forms. */
int64_t genie_match_stats_min_occ_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags);
int genie_match_stats_min_occ(const genie_index *ix, int32_t flags, int32_t min_occ, const uint8_t *d_bases,
                              const int64_t *d_read_offsets, int64_t N, int64_t total_bases, int64_t max_len,
                              int32_t *d_ms,           /* S * total_bases */
                              int32_t *d_lohi,         /* 2 * S * total_bases, may be NULL */
                              int32_t *d_status,       /* S * N, may be NULL */
                              int64_t *d_totals,       /* 1, may be NULL: positions with ms_k < ms */
                              void *d_workspace, int64_t workspace_bytes, void *stream);
int64_t genie_find_smems_min_occ_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags);
int genie_find_smems_min_occ(const genie_index *ix, int32_t mode, int32_t flags, const uint8_t *d_bases,
                             const int64_t *d_read_offsets, int64_t N, int64_t total_bases, int64_t max_len, int32_t min_len,
                             int32_t min_occ,
                             int64_t *d_offsets,      /* S * N + 1 */
                             int32_t *d_rows,         /* 4 * out_cap_rows, 16-byte aligned */
                             int64_t out_cap_rows,
                             int32_t *d_status,       /* S * N, may be NULL */
                             int64_t *d_totals,       /* 1, may be NULL: positions with ms_k < ms */
                             void *d_workspace, int64_t workspace_bytes, void *stream);

/* Reads from TEXT, on the device: the bytes of a file of reads -> the d_bases / d_read_offsets that genie_find_smems_long_ex
 * takes.  The reference has no counterpart (its reads are Python strings); this replaces encoding every string on the host.
 * Lines.  A line ends at a '\n' (0x0A), which is not part of it; if the line is then not empty and its last byte is '\r',
 *   that one byte is dropped too.  The bytes behind the last '\n' are the tail: without GENIE_TEXT_PARTIAL a non-empty tail
 *   is one more line (no '\r' is dropped from it), with GENIE_TEXT_PARTIAL the tail is not a line.  An empty text has no
 *   lines, "\n\n" two empty ones.
 * format GENIE_TEXT_LINES: read r is line r, N = the number of lines; an empty line is a read of length 0.
 * format GENIE_TEXT_FASTQ: record r is lines 4r .. 4r+3, read r is line 4r+1, N = floor(lines / 4).  Line 4r must be non-empty
 *   and start with '@', line 4r+2 non-empty and start with '+': otherwise GENIE_E_INVALID (found on the device) and out5[4] =
 *   the first such record.  Quality lines are not looked at (they may start with '@' and hold '+').  Without
 *   GENIE_TEXT_PARTIAL a number of lines that is no multiple of 4 is GENIE_E_INVALID with out5[4] = N, the incomplete record;
 *   with it the lines of an incomplete last record are not consumed.  Sequences wrapped over several lines are NOT handled:
 *   every record is exactly four lines (FASTA has an entry point of its own, genie_reads_from_fasta below).
 * Translation: an output byte is code_of_byte[b] where that is 0..3, else 4 (a break for GENIE_READS_SPLIT_BREAKS,
 *   GENIE_READ_BAD_BASE without it); never above 4.  Every byte value is legal inside a line except '\n'.  code_of_byte is a
 *   host array of 256 entries, read before the call returns (it travels as a kernel argument).
 * Output: d_bases = the reads' codes back to back, d_read_offsets[0 .. N] their int64 offsets, d_read_offsets[0] = 0;
 *   out5 (host) = {N, total_bases, longest read, consumed_bytes, first bad record or -1}.  consumed_bytes is text_bytes
 *   without GENIE_TEXT_PARTIAL; with it, where the first line that was not consumed starts (GENIE_TEXT_LINES: behind the last
 *   '\n'; GENIE_TEXT_FASTQ: the start of line 4N), so that parsing text[consumed_bytes:] followed by the rest of the stream
 *   continues exactly where this chunk stopped.
 * Sizing: with d_bases and d_read_offsets both NULL only out5 is produced (the capacities are then not looked at).
 *   Otherwise N > cap_reads or total_bases > cap_bases gives GENIE_E_CAPACITY: out5 holds the true values, d_bases is not
 *   written and nothing is written outside d_bases[0 .. cap_bases) and d_read_offsets[0 .. cap_reads] (whose contents are then
 *   undefined).  cap_bases = text_bytes and cap_reads = text_bytes always suffice.  A malformed record is reported before
 *   a capacity.
 * Checked before any device work: GENIE_E_INVALID for a null d_text with text_bytes > 0, a null code_of_byte or out5, a negative
 *   size, an unknown format or flag bit, exactly one of d_bases / d_read_offsets null, d_read_offsets not 8-byte aligned;
 *   then GENIE_E_CAPACITY for a d_tmp that is null, not 256-byte aligned or smaller than
 *   genie_reads_from_text_tmp_bytes(text_bytes, cap_reads) (32 bytes per 4096 of text and 8 per 1024 reads of capacity;
 *   GENIE_E_INVALID for a negative argument).  d_text and d_bases need no alignment.
 * All launches go to `stream` on the current device; the call synchronises it exactly once, at the end (out5 has to reach
 *   the host).  Three streaming passes over the text, nothing per read; the output is a function of the inputs alone. */
#define GENIE_TEXT_LINES 0      /* every line is a read */
#define GENIE_TEXT_FASTQ 1      /* records of four lines; line 2 of each is the read */
#define GENIE_TEXT_PARTIAL 1    /* flags: the text is a chunk of a longer stream */
int64_t genie_reads_from_text_tmp_bytes(int64_t text_bytes, int64_t cap_reads);
int genie_reads_from_text(const uint8_t *d_text, int64_t text_bytes, int32_t format, int32_t flags,
                          const uint8_t *code_of_byte /* host, 256 entries */,
                          uint8_t *d_bases, int64_t cap_bases,
                          int64_t *d_read_offsets, int64_t cap_reads,
                          int64_t *out5 /* host */,
                          void *d_tmp, int64_t tmp_bytes, void *stream);

/* Reads from FASTA text, on the device: '>' header lines, each followed by a sequence wrapped over any number of lines.
 * Lines, the tail, GENIE_TEXT_PARTIAL and the translation through code_of_byte are those of genie_reads_from_text.
 * A header line is a non-empty line whose first byte is '>'; every other line is a sequence line (there is no comment
 *   syntax: a line that starts with ';' is a sequence line).  A '>' elsewhere in a line is an ordinary byte.
 * Record r starts at the r-th header line and runs to just before the next header line or the end of the text.  Read r is
 *   the bytes of its sequence lines, concatenated in order (each without its '\n' and the dropped '\r'; empty lines
 *   contribute nothing); a record without sequence bytes is a read of length 0.
 * With H header lines: without GENIE_TEXT_PARTIAL N = H and consumed_bytes = text_bytes.  With it the last record may go on
 *   in the next chunk: N = max(H - 1, 0) and consumed_bytes = the text position of the last header line's '>' (0 when
 *   H = 0); the bytes from there on are left alone, so that parsing text[consumed_bytes:] followed by the rest of the stream
 *   continues exactly where this chunk stopped.
 * Malformed: a non-empty line in front of the first header line (without GENIE_TEXT_PARTIAL the tail counts).  Then
 *   GENIE_E_INVALID, found on the device, with out5[4] = 0; the outputs' contents are undefined, nothing outside the
 *   capacities is written, and it is reported before a capacity.  Leading empty lines are fine; a text without any
 *   non-empty line is N = 0 and GENIE_OK.
 * Output: d_bases = the reads' codes back to back; d_read_offsets[0 .. N] their int64 offsets, [0] = 0;
 *   d_record_starts[0 .. N) (may be NULL) the text position of every record's '>', for a caller that kept the text and
 *   wants the names; out5 (host) = {N, total_bases, longest read, consumed_bytes, 0 when malformed else -1}.
 * Sizing, capacities, argument checks and synchronisation are word for word those of genie_reads_from_text (the sizing call
 *   has d_bases, d_read_offsets and d_record_starts all NULL; d_record_starts is 8-byte aligned like d_read_offsets and
 *   holds cap_reads entries); the scratch is genie_reads_from_fasta_tmp_bytes(text_bytes, cap_reads), 48 bytes per 4096 of
 *   text.  Three streaming passes over the text, nothing per record and nothing per line, no atomics: the output is a
 *   function of the inputs alone. */
int64_t genie_reads_from_fasta_tmp_bytes(int64_t text_bytes, int64_t cap_reads);
int genie_reads_from_fasta(const uint8_t *d_text, int64_t text_bytes, int32_t flags,
                           const uint8_t *code_of_byte /* host, 256 entries */,
                           uint8_t *d_bases, int64_t cap_bases,
                           int64_t *d_read_offsets, int64_t *d_record_starts /* may be NULL */, int64_t cap_reads,
                           int64_t *out5 /* host */,
                           void *d_tmp, int64_t tmp_bytes, void *stream);

/* A reference with AMBIGUOUS BASES (N runs, IUPAC codes), cut into segments on the device.  genie_index_create* refuses a
 * code > 3 (GENIE_E_ALPHABET) and keeps doing so.  Instead every break is removed, the index is built over what is left,
 * the SQUEEZED concatenation, the maximal A/C/G/T runs go to the *_contigs calls as the contig table -- no match covers a
 * break or runs from one side of it to the other, which is what those calls guarantee for contig boundaries -- and
 * genie_segment_coords names every position in the coordinates of the reference as it was given, breaks counted.
 * Definitions.  The GIVEN reference is d_codes[0 .. n_given) (uint8, any alignment) with a record table d_record_offsets:
 *   n_records + 1 int64 values on the device, 8-byte aligned, by the contig-table convention (off[0] = 0, non-decreasing,
 *   off[n_records] = n_given; record r is [off[r], off[r+1]), empty records allowed; the record of position i is the last
 *   r with off[r] <= i).  d_record_offsets == NULL is allowed with n_records == 1 and means one record [0, n_given).
 * A BREAK is a position whose code is > 3 (any byte 4 .. 255): the convention of the read calls and of what
 *   genie_reads_from_fasta's translation leaves for a letter that is no base.
 * A SEGMENT is a maximal run of non-break positions inside one record: it ends at a break, at its record's end or at
 *   n_given.  Segments are numbered in the order of their positions.  A record without a kept base has no segment; the
 *   other segments still carry their record's number.
 * Outputs:
 *   d_bases            the stream compaction of the non-break bytes: the squeezed concatenation (n_kept bytes);
 *   d_seg_offsets[s]   the kept bytes in front of segment s, [n_seg] = n_kept: a valid contig table of d_bases;
 *   d_seg_record[s]    the record of segment s;  d_seg_origin[s]  the 0-based offset of its first base INSIDE that record;
 *   out4 (host)        {n_seg, n_kept, longest segment, table error mask}: the mask is 0 for a valid table, else bit 1 for
 *                      off[0] != 0, 2 for a decrease, 4 for off[n_records] != n_given (genie_contigs_validate's conditions).
 * Sizing: with all four output pointers NULL only out4 is produced and the capacities are not looked at.  Otherwise
 *   n_seg > cap_segs or n_kept > cap_bases gives GENIE_E_CAPACITY: out4 holds the true values and nothing is stored
 *   (d_seg_offsets holds cap_segs + 1 values).  cap_bases = n_given and cap_segs = (n_given + 1) / 2 suffice for ONE record;
 *   a record boundary without a break on it starts a segment too, so with records cap_segs = n_given always suffices.
 * A bad table gives GENIE_E_INVALID, found on the device and reported before a capacity, with its bits in out4[3] and
 *   out4[0 .. 2] = 0; nothing is stored, and no load leaves d_codes or the table whatever the table holds.
 * Checked before any device work, GENIE_E_INVALID: a null d_codes with n_given > 0, a null out4, a negative n_given,
 *   tmp_bytes or (unless sizing) capacity, n_records < 1, a NULL table with n_records != 1, some but not all output
 *   pointers NULL, a table, d_seg_offsets or d_seg_origin that is not 8-byte or a d_seg_record that is not 4-byte aligned;
 *   GENIE_E_TOO_LONG for n_records above 2^31 - 1 (d_seg_record is int32); then GENIE_E_CAPACITY for a d_tmp that is null,
 *   not 256-byte aligned or smaller than genie_reference_segments_tmp_bytes(n_given, n_records): 32 bytes per 4096 of given
 *   reference, nothing per record; GENIE_E_INVALID for a negative argument, a multiple of 256, monotone in both.
 * Every position, n_given included, is 64-bit; n_kept >= 2^31 is reported as it is (the index builder refuses it, not the
 *   squeeze).  `stream` is synchronised once, at the end.  Two streaming passes over the given codes in tiles of 4096
 *   bytes; the record boundaries inside a tile are resolved once per tile (two bisections of the table, then one bit per
 *   boundary in LDS), nothing per byte.  No atomic decides a value: the outputs are a function of the inputs alone. */
int64_t genie_reference_segments_tmp_bytes(int64_t n_given, int64_t n_records);
int genie_reference_segments(const uint8_t *d_codes, int64_t n_given,
                             const int64_t *d_record_offsets /* may be NULL */, int64_t n_records,
                             uint8_t *d_bases, int64_t cap_bases,
                             int64_t *d_seg_offsets /* cap_segs + 1 */, int32_t *d_seg_record, int64_t *d_seg_origin,
                             int64_t cap_segs,
                             int64_t *out4 /* host */,
                             void *d_tmp, int64_t tmp_bytes, void *stream);

/* Squeezed coordinates -> coordinates in the GIVEN reference.  ix: the index over d_bases; the three segment arrays as
 * genie_reference_segments wrote them, n_segs = n_seg.  Input, int32, element i at d_in[i * stride]:
 *   GENIE_SEG_POSITIONS  a 1-based position in the squeezed concatenation (MEM rows' pos with stride 4, genie_locate);
 *   GENIE_SEG_HITS       d_in[i*stride], d_in[i*stride + 1] = (segment, 1-based offset inside it): the hits of
 *                        genie_locate_contigs with the segment table; stride >= 2.
 * Output d_out[2 i], d_out[2 i + 1] (int64, 16-byte aligned) = (record, 1-based offset inside the GIVEN record, breaks
 * counted) = (d_seg_record[s], d_seg_origin[s] + offset in segment s); (-1, -1) for a position outside [1, n], a segment
 * outside [0, n_segs) or an offset outside its segment.  The positions form finds s with the LDS-staged bisection of the
 * contig calls; the hits form is a gather.  One lane per element, no synchronisation of `stream`.
 * Checks, before the device check: a null ix, an unknown form, count < 0, stride < 1 (< 2 for hits), a null d_in or
 * d_out with count > 0, a d_in that is not 4-byte or a d_out that is not 16-byte aligned, a null or misaligned segment
 * array or n_segs < 1 give GENIE_E_INVALID, n_segs above 2^31 - 2 GENIE_E_TOO_LONG.  d_seg_record is only copied, never
 * followed; the call is memory-safe on any table contents (undefined values for a table genie_contigs_validate refuses). */
#define GENIE_SEG_POSITIONS 0
#define GENIE_SEG_HITS 1
int genie_segment_coords(const genie_index *ix, const int64_t *d_seg_offsets, const int32_t *d_seg_record,
                         const int64_t *d_seg_origin, int64_t n_segs, int32_t form,
                         const int32_t *d_in, int32_t stride, int64_t count,
                         int64_t *d_out /* 2 * count, 16-byte aligned */, void *stream);

/* The same discovery for callers on the far side of a host link (SMEM.find_smems_* on host arrays): 2-bit packed reads in,
 * 8-byte rows out -- 40 instead of 150 bytes per 150-base read over PCIe, 8 instead of 16 per SMEM.  Reads of at most 255
 * bases.  Row r of d_reads2bit = stride_bytes bytes (a multiple of 4, >= 4 * ceil(max length / 16)): byte i holds bases
 * 4i .. 4i+3, base 4i in bits 7..6 (codes as above; bases past the read's length are ignored).  Output:
 *   d_counts8[r]  SMEMs of read r (flagged reads: 0);  d_status8[r] = its GENIE_READ_* code;
 *   d_rows8       dense, reads in input order, SMEMs in emission order (the CSR rows of genie_find_smems_csr; a read's
 *                 rows start at the sum of the counts before it), 8 bytes each: byte 0 start, byte 1 end, bytes 2..3
 *                 span = hi - lo (little endian), bytes 4..7 lo.  span == 0xFFFF means "65535 or more": that row's
 *                 index and its hi are also appended to d_escapes (int64 pairs: row, hi; unordered);
 *   d_totals[0]   rows in all (rows beyond out_cap_rows were dropped);  d_totals[1] = escapes in all, of the rows that
 *                 were not dropped (compare with cap_escapes and call again with a larger list if it is exceeded).
 * The reference has no counterpart (its API is in-process Python strings); genie-smem_amd/packing.py holds the host side:
 * pack_reads() and unpack_rows() give back exactly the int32 (start, end, lo, hi) rows of genie_find_smems_csr. */
int genie_find_smems_packed(const genie_index *ix, int32_t mode, const uint8_t *d_reads2bit, const int32_t *d_lens, int64_t N,
                            int32_t stride_bytes, int32_t fixed_len, int32_t min_len, uint8_t *d_counts8, uint8_t *d_status8,
                            void *d_rows8, int64_t out_cap_rows, int64_t *d_totals, int64_t *d_escapes, int64_t cap_escapes,
                            void *d_workspace, int64_t workspace_bytes, void *stream);

/* The same with 6-byte rows (another quarter off the bytes that travel back: 66 instead of 88 per 150-base read), for
 * references below 2^24 bases (GENIE_E_TOO_LONG otherwise): byte 0 start, byte 1 end, bytes 2..4 lo (24 bits, little endian),
 * byte 5 span = hi - lo, 0xFF meaning "255 or more" (that row's index and hi are on d_escapes).  d_rows6: 2-byte aligned.
 * Everything else as genie_find_smems_packed; packing.unpack_rows(..., row_bytes=6) is the host side.
 * Alignment (GENIE_E_INVALID otherwise): d_reads2bit 4 bytes (rows of 32-bit words), d_rows8 8, d_totals 8. */
int genie_find_smems_packed6(const genie_index *ix, int32_t mode, const uint8_t *d_reads2bit, const int32_t *d_lens, int64_t N,
                             int32_t stride_bytes, int32_t fixed_len, int32_t min_len, uint8_t *d_counts8, uint8_t *d_status8,
                             void *d_rows6, int64_t out_cap_rows, int64_t *d_totals, int64_t *d_escapes, int64_t cap_escapes,
                             void *d_workspace, int64_t workspace_bytes, void *stream);

/* Compact the slotted output to CSR: d_offsets[N+1] (exclusive prefix sum of min(count,cap))
 * and d_out[total*4].  d_out may be NULL (offsets only: the sizing call); rows beyond out_cap_rows are dropped
 * (d_offsets[N] still holds the true total).  d_slots and d_out 16-byte aligned; d_tmp: 8-byte aligned scratch of
 * genie_compact_tmp_bytes(N) bytes. */
int64_t genie_compact_tmp_bytes(int64_t N);
int genie_compact_smems(const int32_t *d_counts, const int32_t *d_slots, int64_t N, int32_t cap,
                        int64_t *d_offsets, int32_t *d_out, int64_t out_cap_rows, void *d_tmp, void *stream);

/* Rows -> reference coordinates: ExactMatch.get_positions (SMEM/ExactMatch.py:195-199) for S intervals at
 * once.  Interval t is (d_lohi[t*stride], d_lohi[t*stride + 1]) = inclusive rows (lo, hi); lo < 0 or
 * hi < lo (absent) contributes nothing.  Pass the (lo, hi) columns of a find_smems result as
 * d_rows + 2 with stride 4, or a genie_sa_interval result with stride 2.  Output CSR:
 * d_pos_offsets[S+1], d_positions[...] = the suffix-array entries of rows lo..hi, 1-based like the
 * reference's, in row order (ExactMatch.exact_match sorts them: :174-192).  Entries beyond cap_positions
 * are dropped (compare d_pos_offsets[S] with the capacity).  d_tmp: 256-byte aligned scratch of
 * genie_locate_tmp_bytes(S) bytes. */
int64_t genie_locate_tmp_bytes(int64_t S);
int genie_locate(const genie_index *ix, const int32_t *d_lohi, int32_t stride, int64_t S, int64_t *d_pos_offsets,
                 int32_t *d_positions, int64_t cap_positions, void *d_tmp, int64_t tmp_bytes, void *stream);

/* Launch-time options of an index handle (none of them changes results).
 * GENIE_OPT_SEARCH_ALL (default 0): the matching statistics fwd[] are non-decreasing along a read, so by default
 *   the match-statistics kernel looks up every 4th position and the three between two of them only where their
 *   values differ.  Value 1 looks up every position (differential testing, A/B timing).
 * GENIE_OPT_GROUP_POSITIONS (default 0 = built-in): read positions a wave works on per iteration (tuning).
 * GENIE_OPT_SEARCH_BLOCKS_PER_CU (default 0 = as many as fit): cap on resident blocks of that kernel (tuning).
 * GENIE_OPT_SEARCH_ONLY (default 0): launch the match-statistics kernel only -- outputs are NOT produced and the
 *   find_smems entry points return GENIE_W_SEARCH_ONLY instead of GENIE_OK; for timing that kernel alone.
 * GENIE_OPT_SEARCH_STAGES_OFF (default 0; honoured only while GENIE_OPT_SEARCH_ONLY is set, so never on a run that
 *   produces output): bit mask of stages of that kernel to skip -- 1 slow list, 2 round 2, 4 rounds 1+2, 8 packed-read
 *   records, 32 fwd rows; the stage ablation of DESIGN.md section 4 (tools/ka_sweep.sh).
 * GENIE_OPT_SCHEDULING (default 0; A/B timing, results unchanged): bit mask -- 1: the match-statistics kernel gives every
 *   wave a fixed share of the read groups instead of handing them out per block; 2: its waves keep one issue priority
 *   instead of rotating it; 4: the same for the interval kernel; 8: the match-statistics kernels do not ask for their next
 *   group's input rows through the scalar cache ahead of time. */
enum { GENIE_OPT_SEARCH_ALL = 2, GENIE_OPT_GROUP_POSITIONS = 4, GENIE_OPT_SEARCH_ONLY = 5, GENIE_OPT_SEARCH_BLOCKS_PER_CU = 6,
       GENIE_OPT_SEARCH_STAGES_OFF = 7, GENIE_OPT_SCHEDULING = 8 };
int genie_index_set_option(genie_index *ix, int32_t option, int32_t value);

/* Profiling hook: two hipEvent_t (as void*, created by the caller with timing enabled) that the next
 * genie_find_smems calls record on their stream immediately before and after the dominant kernel of
 * the path (the match-statistics kernel, match_table_kernel / match_table_long_kernel).
 * Pass NULLs to stop.  Not thread-safe with concurrent launches on the same handle. */
int genie_index_set_stage_events(genie_index *ix, void *ev_search_begin, void *ev_search_end);

/* Launch geometry actually used by genie_find_smems for (mode, max read length): for reports. */
int genie_launch_info(const genie_index *ix, int32_t mode, int32_t max_len, int32_t *grid, int32_t *block,
                      int32_t *lds_bytes);

/* Name of the match-statistics (dominant) kernel genie_find_smems launches for (mode, max read length), as a
 * profiler prints it without the argument list: for reports that look the kernel up in a rocprofv3 trace. */
int genie_search_kernel_name(const genie_index *ix, int32_t mode, int32_t max_len, char *buf, int32_t cap);

const char *genie_strerror(int status);
const char *genie_last_hip_error(void);
int genie_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GENIE_SMEM_H */

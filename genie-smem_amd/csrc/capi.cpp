// capi.cpp -- the extern "C" surface declared in include/genie_smem.h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <new>

#include "genie_internal.h"

using namespace genie;

namespace {

int check_hip(hipError_t e, const char *what)
{
    if (e == hipSuccess) return GENIE_OK;
    set_hip_error(what, (int)e);
    return GENIE_E_HIP;
}

int query_cus(int device)
{
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
    return cus;
}

int make_index(const uint8_t *codes, int64_t n, const int32_t *sa1, int32_t K, int32_t P, int32_t P2, int32_t fmt, genie_index **out)
{
    if (!out) return GENIE_E_INVALID;
    HostIndex *h = nullptr;
    int rc = build_host_index(codes, n, sa1, K, P, P2, fmt, &h);
    if (rc) return rc;
    genie_index *ix = new (std::nothrow) genie_index();
    if (!ix) { delete h; return GENIE_E_NOMEM; }
    ix->host = h;
    fill_header(*h, &ix->hdr);
    ix->has_hdr = true;
    *out = ix;
    return GENIE_OK;
}

// genie_index_create_ex's parameter rules; P, P2 and the table form of a build with these arguments
int device_params(int64_t n, int32_t K, int32_t dir_bits, int32_t table_bits, int32_t *P, int32_t *P2, bool *compact)
{
    *P = (dir_bits <= 0 || dir_bits > GENIE_MAX_DIR_BITS) ? GENIE_MAX_DIR_BITS : dir_bits;
    const int32_t fmt = table_bits >> 8;
    table_bits &= 0xFF;
    if (fmt < 0 || fmt > 2) return GENIE_E_INVALID;
    if (table_bits != 0 && (table_bits <= *P || table_bits > 12)) return GENIE_E_INVALID;
    if (n < 1 || n > 0x7ffffff0ll || K < 0 || K > GENIE_MAX_K) return GENIE_E_INVALID;
    if (fmt == 2 && n >= kM16MaxN) return GENIE_E_INVALID;
    *P2 = choose_p2(n, *P, table_bits);
    *compact = fmt == 2 || (fmt == 0 && n < kM16MaxN);
    return GENIE_OK;
}
}  // namespace

static int ready(const genie_index *ix);

extern "C" {

int genie_abi_version(void) { return GENIE_ABI_VERSION; }

int genie_index_create(const uint8_t *codes, int64_t n, int32_t K, int32_t dir_bits, genie_index **out)
{
    return make_index(codes, n, nullptr, K, dir_bits, 0, 0, out);
}

int genie_index_create_ex(const uint8_t *codes, int64_t n, const int32_t *sa_one_based, int32_t K, int32_t dir_bits,
                          int32_t table_bits, genie_index **out)
{
    const int32_t P = (dir_bits <= 0 || dir_bits > GENIE_MAX_DIR_BITS) ? GENIE_MAX_DIR_BITS : dir_bits;   // as build_host_index
    const int32_t fmt = table_bits >> 8;                      // GENIE_TABLE_WIDE / GENIE_TABLE_COMPACT, 0 = automatic
    table_bits &= 0xFF;
    if (fmt < 0 || fmt > 2) return GENIE_E_INVALID;
    if (table_bits != 0 && (table_bits <= P || table_bits > 12)) return GENIE_E_INVALID;
    return make_index(codes, n, sa_one_based, K, dir_bits, table_bits, fmt, out);
}

int genie_index_create_from_sa(const uint8_t *codes, int64_t n, const int32_t *sa_one_based, int32_t K,
                               int32_t dir_bits, genie_index **out)
{
    if (!sa_one_based) return GENIE_E_INVALID;
    return make_index(codes, n, sa_one_based, K, dir_bits, 0, 0, out);
}

int genie_index_set_rmi(genie_index *ix, int32_t nlev, const int32_t *sizes, const int32_t *scales,
                        const double *coef, const double *icpt)
{
    if (!ix || !ix->host || ix->has_dev) return GENIE_E_INVALID;
    if (nlev < 1 || nlev > GENIE_MAX_RMI_LEVELS || !sizes || !scales || !coef || !icpt) return GENIE_E_INVALID;
    if (sizes[0] != 1) return GENIE_E_INVALID;
    HostIndex &h = *ix->host;
    int64_t tot = 0;
    for (int l = 0; l < nlev; l++) {
        if (sizes[l] < 1 || scales[l] < 1) return GENIE_E_INVALID;
        if (l + 1 < nlev && sizes[l + 1] != scales[l]) return GENIE_E_INVALID;   // next level has `scale` experts
        tot += sizes[l];
    }
    h.nlev = nlev;
    int64_t off = 0;
    for (int l = 0; l < GENIE_MAX_RMI_LEVELS; l++) {
        h.rmi_size[l] = l < nlev ? sizes[l] : 0;
        h.rmi_scale[l] = l < nlev ? scales[l] : 0;
        h.rmi_off[l] = (int32_t)off;
        if (l < nlev) off += sizes[l];
    }
    h.rmi_off[GENIE_MAX_RMI_LEVELS] = (int32_t)off;
    for (int l = nlev; l <= GENIE_MAX_RMI_LEVELS; l++) h.rmi_off[l] = (int32_t)tot;
    h.rmi.resize((size_t)tot);
    for (int64_t i = 0; i < tot; i++) h.rmi[(size_t)i] = RmiModel{coef[i], icpt[i]};
    h.rmi_err.clear();                       // error bounds belong to a natively trained model
    fill_header(h, &ix->hdr);
    return GENIE_OK;
}

int genie_index_train_rmi(genie_index *ix, int32_t n_experts, const int32_t *experts, double *mean_abs_err,
                          int32_t *max_abs_err)
{
    if (!ix || !ix->host || ix->has_dev || (n_experts > 0 && !experts)) return GENIE_E_INVALID;
    int rc = train_rmi(*ix->host, n_experts, experts, mean_abs_err, max_abs_err);
    if (rc) return rc;
    fill_header(*ix->host, &ix->hdr);
    return GENIE_OK;
}

int genie_index_rmi_models(const genie_index *ix, double *coef, double *icpt, int32_t *leaf_err)
{
    if (!ix || !ix->host || ix->host->nlev < 1) return GENIE_E_INVALID;
    const HostIndex &h = *ix->host;
    for (size_t i = 0; i < h.rmi.size(); i++) {
        if (coef) coef[i] = h.rmi[i].coef;
        if (icpt) icpt[i] = h.rmi[i].icpt;
    }
    if (leaf_err) {
        if (h.rmi_err.empty()) return GENIE_E_INVALID;
        for (size_t i = 0; i < h.rmi_err.size(); i++) leaf_err[i] = h.rmi_err[i];
    }
    return GENIE_OK;
}

int genie_index_info(const genie_index *ix, genie_info *out)
{
    if (!ix || !out || !ix->has_hdr) return GENIE_E_INVALID;
    out->n = ix->hdr.n;
    out->K = ix->hdr.K;
    out->dir_bits = ix->hdr.P;
    out->lut_keys = ix->hdr.lut_keys;
    out->lut_slots = ix->hdr.lut_slots;
    out->rmi_levels = ix->hdr.nlev;
    out->has_host = ix->host != nullptr;
    out->has_device = ix->has_dev;
    out->device = ix->device;
    out->blob_bytes = ix->hdr.total_bytes;
    return GENIE_OK;
}

const int32_t *genie_index_suffix_array(const genie_index *ix)
{
    return (ix && ix->host) ? ix->host->sa1.data() : nullptr;
}

int genie_index_lut_arrays(const genie_index *ix, const uint32_t **codes, const int32_t **lo, const int32_t **hi)
{
    if (!ix || !ix->host) return GENIE_E_INVALID;
    if (codes) *codes = ix->host->lut_code.data();
    if (lo) *lo = ix->host->lut_lo.data();
    if (hi) *hi = ix->host->lut_hi.data();
    return GENIE_OK;
}

int64_t genie_index_blob_bytes(const genie_index *ix)
{
    return (ix && ix->has_hdr) ? ix->hdr.total_bytes : (int64_t)GENIE_E_INVALID;
}

int genie_index_serialize(const genie_index *ix, void *host_dst, int64_t cap)
{
    if (!ix || !ix->host) return GENIE_E_INVALID;
    return serialize(*ix->host, host_dst, cap);
}

int64_t genie_index_image_bytes(const genie_index *ix, int32_t image_flags)
{
    if (!ix || !ix->host || (image_flags & ~GENIE_IMAGE_NO_SEED_TABLE)) return (int64_t)GENIE_E_INVALID;
    BlobHeader hdr;
    fill_header(*ix->host, &hdr, image_flags);
    return hdr.total_bytes;
}

int genie_index_serialize_image(const genie_index *ix, int32_t image_flags, void *host_dst, int64_t cap)
{
    if (!ix || !ix->host || (image_flags & ~GENIE_IMAGE_NO_SEED_TABLE)) return GENIE_E_INVALID;
    return serialize(*ix->host, host_dst, cap, image_flags);
}

int genie_index_open(const void *host_header, const void *d_blob, int64_t blob_bytes, int32_t device,
                     genie_index **ix_inout)
{
    if (!host_header || !d_blob || !ix_inout) return GENIE_E_INVALID;
    BlobHeader hdr;
    memcpy(&hdr, host_header, sizeof(hdr));
    DevIndex dev;
    int rc = dev_index_from_header(hdr, d_blob, blob_bytes, &dev);
    if (rc) return rc;
    genie_index *ix = *ix_inout;
    if (!ix) {
        ix = new (std::nothrow) genie_index();
        if (!ix) return GENIE_E_NOMEM;
    }
    ix->hdr = hdr;
    ix->has_hdr = true;
    ix->dev = dev;
    ix->has_dev = true;
    ix->device = device;
    ix->blob_bytes = blob_bytes;
    ix->num_cus = query_cus(device);
    *ix_inout = ix;
    return GENIE_OK;
}

int genie_index_validate(const genie_index *ix, uint32_t *what, void *stream)
{
    int rc = ready(ix);
    if (rc) return rc;
    unsigned int w = 0;
    rc = validate_image(ix, &w, stream);
    if (what) *what = w;
    return rc;
}

int genie_index_to_device(genie_index *ix, int32_t device)
{
    if (!ix || !ix->host) return GENIE_E_INVALID;
    int rc = check_hip(hipSetDevice(device), "hipSetDevice");
    if (rc) return rc;
    const int64_t bytes = ix->hdr.total_bytes;
    void *host = malloc((size_t)bytes);
    if (!host) return GENIE_E_NOMEM;
    rc = serialize(*ix->host, host, bytes);
    void *d = nullptr;
    if (!rc) rc = check_hip(hipMalloc(&d, (size_t)bytes), "hipMalloc(index image)");
    if (!rc) rc = check_hip(hipMemcpy(d, host, (size_t)bytes, hipMemcpyHostToDevice), "hipMemcpy(index image)");
    if (!rc) {
        if (ix->owned_blob) (void)hipFree(ix->owned_blob);
        ix->owned_blob = d;
        rc = genie_index_open(host, d, bytes, device, &ix);
    } else if (d) {
        (void)hipFree(d);
    }
    free(host);
    return rc;
}


int64_t genie_index_device_image_bound(int64_t n, int32_t K, int32_t dir_bits, int32_t table_bits)
{
    int32_t P, P2;
    bool compact;
    const int rc = device_params(n, K, dir_bits, table_bits, &P, &P2, &compact);
    return rc ? (int64_t)rc : device_image_bound(n, K, P, P2, compact);
}

int64_t genie_index_device_build_tmp_bytes(int64_t n, int32_t K, int32_t dir_bits, int32_t table_bits)
{
    int32_t P, P2;
    bool compact;
    const int rc = device_params(n, K, dir_bits, table_bits, &P, &P2, &compact);
    return rc ? (int64_t)rc : device_build_tmp_bytes(n, K, P, P2);
}

int genie_index_create_device(const uint8_t *d_codes, int64_t n, int32_t K, int32_t dir_bits, int32_t table_bits,
                              int32_t image_flags, void *d_image, int64_t image_cap, int64_t *image_bytes, void *d_tmp,
                              int64_t tmp_bytes, int32_t device, void *stream, genie_index **out)
{
    if (!d_codes || !d_image || !image_bytes || !d_tmp || !out) return GENIE_E_INVALID;
    if (image_flags & ~GENIE_IMAGE_NO_SEED_TABLE) return GENIE_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(d_image) & 255) != 0 || (reinterpret_cast<uintptr_t>(d_tmp) & 255) != 0) return GENIE_E_INVALID;
    int32_t P, P2;
    bool compact;
    int rc = device_params(n, K, dir_bits, table_bits, &P, &P2, &compact);
    if (rc) return rc;
    if (image_cap < device_image_bound(n, K, P, P2, compact) || tmp_bytes < device_build_tmp_bytes(n, K, P, P2))
        return GENIE_E_INVALID;
    rc = check_hip(hipSetDevice(device), "hipSetDevice");
    if (rc) return rc;
    BlobHeader hdr;
    rc = device_build(d_codes, n, K, P, P2, compact, image_flags, d_image, image_cap, d_tmp, tmp_bytes, stream, &hdr);
    if (rc) return rc;
    genie_index *ix = nullptr;
    rc = genie_index_open(&hdr, d_image, hdr.total_bytes, device, &ix);
    if (rc) return rc;
    *image_bytes = hdr.total_bytes;
    *out = ix;
    return GENIE_OK;
}

void genie_index_destroy(genie_index *ix)
{
    if (!ix) return;
    if (ix->owned_blob) (void)hipFree(ix->owned_blob);
    delete ix->host;
    delete ix;
}

static int ready(const genie_index *ix)
{
    if (!ix) return GENIE_E_INVALID;
    if (!ix->has_dev) return GENIE_E_NO_DEVICE;
    return GENIE_OK;
}

// the tables an SMEM search of `mode` needs: the K-mer table (LUT / RMI) and the model (RMI)
static int mode_tables(const genie_index *ix, int32_t mode)
{
    if (mode != GENIE_MODE_BWA && ix->dev.K < 1) return GENIE_E_NO_LUT;
    return mode == GENIE_MODE_RMI && ix->dev.nlev < 1 ? GENIE_E_NO_MODEL : GENIE_OK;
}

int genie_sa_interval(const genie_index *ix, const uint8_t *d_pats, const int32_t *d_lens, int64_t N,
                      int32_t stride, int32_t fixed_len, int32_t *d_out_lohi, void *stream)
{
    int rc = ready(ix);
    if (rc) return rc;
    if (N < 0 || stride < 0 || fixed_len < 0 || (N > 0 && (!d_pats || !d_out_lohi))) return GENIE_E_INVALID;
    if (fixed_len > GENIE_MAX_READ_LEN) return GENIE_E_TOO_LONG;
    return launch_sa_interval(ix, d_pats, d_lens, N, stride, fixed_len, d_out_lohi, stream);
}

int genie_seed_lookup(const genie_index *ix, int32_t mode, const uint8_t *d_kmers, int64_t N,
                      int32_t *d_out_lohi, double *d_pred, void *stream)
{
    int rc = ready(ix);
    if (rc) return rc;
    if (N < 0 || (N > 0 && (!d_kmers || !d_out_lohi))) return GENIE_E_INVALID;
    if (ix->dev.K < 1) return GENIE_E_NO_LUT;
    if (mode == GENIE_MODE_LUT && (ix->dev.flags & kFlagNoSeedTable)) return GENIE_E_NO_LUT;     // a find_smems-only image
    if (mode == GENIE_MODE_RMI && ix->dev.nlev < 1) return GENIE_E_NO_MODEL;
    return launch_seed_lookup(ix, mode, d_kmers, N, d_out_lohi, d_pred, stream);
}

int genie_find_smems(const genie_index *ix, int32_t mode, const uint8_t *d_reads, const int32_t *d_lens,
                     int64_t N, int32_t stride, int32_t fixed_len, int32_t min_len, int32_t *d_counts,
                     int32_t *d_slots, int32_t cap, int32_t *d_status, void *d_workspace, int64_t workspace_bytes,
                     void *stream)
{
    int rc = ready(ix);
    if (rc) return rc;
    if (N < 0 || stride < 0 || fixed_len < 0 || cap < 1 || (N > 0 && (!d_reads || !d_counts || !d_slots)))
        return GENIE_E_INVALID;
    if (mode < GENIE_MODE_BWA || mode > GENIE_MODE_RMI) return GENIE_E_INVALID;
    if (fixed_len > GENIE_MAX_READ_LEN) return GENIE_E_TOO_LONG;
    if ((rc = mode_tables(ix, mode))) return rc;
    if ((reinterpret_cast<uintptr_t>(d_slots) & 15) != 0) return GENIE_E_INVALID;
    return launch_find_smems(ix, mode, {d_reads, d_lens, N, stride, fixed_len, min_len, d_status, d_workspace, workspace_bytes},
                             d_counts, d_slots, cap, stream);
}

int genie_find_smems_csr(const genie_index *ix, int32_t mode, const uint8_t *d_reads, const int32_t *d_lens,
                         int64_t N, int32_t stride, int32_t fixed_len, int32_t min_len, int64_t *d_offsets,
                         int32_t *d_rows, int64_t out_cap_rows, int32_t *d_status, void *d_workspace,
                         int64_t workspace_bytes, void *stream)
{
    int rc = ready(ix);
    if (rc) return rc;
    if (N < 0 || stride < 0 || fixed_len < 0 || out_cap_rows < 0 || !d_offsets || (N > 0 && (!d_reads || !d_rows)))
        return GENIE_E_INVALID;
    if (mode < GENIE_MODE_BWA || mode > GENIE_MODE_RMI) return GENIE_E_INVALID;
    if (fixed_len > GENIE_MAX_READ_LEN) return GENIE_E_TOO_LONG;
    if ((rc = mode_tables(ix, mode))) return rc;
    if ((reinterpret_cast<uintptr_t>(d_rows) & 15) != 0) return GENIE_E_INVALID;
    return launch_find_smems_csr(ix, mode, {d_reads, d_lens, N, stride, fixed_len, min_len, d_status, d_workspace, workspace_bytes},
                                 d_offsets, d_rows, out_cap_rows, stream);
}

int64_t genie_find_smems_both_workspace_bytes(int64_t N, int32_t max_len)
{
    if (N < 0 || max_len < 0) return (int64_t)GENIE_E_INVALID;
    if (max_len > GENIE_MAX_READ_LEN) return (int64_t)GENIE_E_TOO_LONG;
    return find_smems_both_workspace_bytes(N, max_len);
}

int genie_find_smems_both(const genie_index *ix, int32_t mode, const uint8_t *d_reads, const int32_t *d_lens, int64_t N,
                          int32_t stride, int32_t fixed_len, int32_t min_len, int64_t *d_offsets, int32_t *d_rows,
                          int64_t out_cap_rows, int32_t *d_status, void *d_workspace, int64_t workspace_bytes, void *stream)
{
    // argument checks first: they need no device image
    if (!ix) return GENIE_E_INVALID;
    if (N < 0 || N > ((int64_t)1 << 40) || stride < 0 || fixed_len < 0 || out_cap_rows < 0 || !d_offsets ||
        (N > 0 && (!d_reads || !d_rows || !d_workspace)))
        return GENIE_E_INVALID;
    if (mode < GENIE_MODE_BWA || mode > GENIE_MODE_RMI) return GENIE_E_INVALID;
    if (fixed_len > GENIE_MAX_READ_LEN) return GENIE_E_TOO_LONG;
    if (N > 0 && stride < fixed_len) return GENIE_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(d_rows) & 15) != 0) return GENIE_E_INVALID;
    if (N > 0 && ((reinterpret_cast<uintptr_t>(d_workspace) & 255) != 0 || workspace_bytes < find_smems_both_workspace_bytes(N, fixed_len)))
        return GENIE_E_CAPACITY;
    int rc = ready(ix);
    if (rc || (rc = mode_tables(ix, mode))) return rc;
    return launch_find_smems_both(ix, mode, {d_reads, d_lens, N, stride, fixed_len, min_len, d_status, d_workspace, workspace_bytes},
                                  d_offsets, d_rows, out_cap_rows, stream);
}

int64_t genie_find_smems_split_workspace_bytes(int64_t N, int32_t max_len)
{
    if (N < 0 || max_len < 0 || max_len > GENIE_MAX_READ_LEN) return (int64_t)GENIE_E_INVALID;
    return find_smems_split_workspace_bytes(N, max_len);
}

int genie_find_smems_split(const genie_index *ix, const uint8_t *d_reads, const int32_t *d_lens, int64_t N, int32_t stride,
                           int32_t fixed_len, int32_t min_len, int64_t *d_offsets, int32_t *d_rows, int64_t out_cap_rows,
                           int32_t *d_status, void *d_workspace, int64_t workspace_bytes, void *stream)
{
    // argument checks first: they need no device image
    if (!ix) return GENIE_E_INVALID;
    if (N < 0 || stride < 0 || fixed_len < 0 || out_cap_rows < 0 || !d_offsets || (N > 0 && (!d_reads || !d_rows || !d_workspace)))
        return GENIE_E_INVALID;
    if (fixed_len > GENIE_MAX_READ_LEN) return GENIE_E_TOO_LONG;
    if (N > 0 && stride < fixed_len) return GENIE_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(d_rows) & 15) != 0 || (reinterpret_cast<uintptr_t>(d_workspace) & 255) != 0) return GENIE_E_INVALID;
    if (N > 0 && workspace_bytes < find_smems_split_workspace_bytes(N, fixed_len)) return GENIE_E_CAPACITY;
    int rc = ready(ix);
    if (rc) return rc;
    return launch_find_smems_split(ix, d_reads, d_lens, N, stride, fixed_len, min_len, d_offsets, d_rows, out_cap_rows, d_status,
                                   d_workspace, workspace_bytes, stream);
}

// the long call is the _ex call with no flags: its checks, in its order, and its launch
int64_t genie_find_smems_long_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len)
{
    return genie_find_smems_long_ex_workspace_bytes(N, total_bases, max_len, 0);
}

int genie_find_smems_long(const genie_index *ix, int32_t mode, const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N,
                          int64_t total_bases, int64_t max_len, int32_t min_len, int64_t *d_offsets, int32_t *d_rows,
                          int64_t out_cap_rows, int32_t *d_status, void *d_workspace, int64_t workspace_bytes, void *stream)
{
    return genie_find_smems_long_ex(ix, mode, 0, d_bases, d_read_offsets, N, total_bases, max_len, min_len, d_offsets, d_rows,
                                    out_cap_rows, d_status, d_workspace, workspace_bytes, stream);
}

// ---- The CSR calls: a batch of reads as one buffer of bases and 64-bit offsets (CsrBatch).  What they check alike is written
// once, below; what a call checks on its own stands in the call.  Everywhere a bad argument (GENIE_E_INVALID, and for a
// contig table GENIE_E_TOO_LONG) comes before a capacity, and the device image and the tables of a mode are looked at last.
constexpr int32_t kReadFlags = GENIE_READS_BOTH_STRANDS | GENIE_READS_SPLIT_BREAKS;

static bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// The sizes and flags of a batch, which the sizing functions take too: no negative count, no read longer than an int
// counts, no flag outside `allowed`
static bool bad_batch(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags, int32_t allowed)
{
    return N < 0 || total_bases < 0 || max_len < 0 || max_len > 0x7fffffffll || (flags & ~allowed) != 0;
}

// ... and the bases and read offsets of a call, where there are any to read
static bool bad_batch(const CsrBatch &b, int32_t allowed)
{
    return bad_batch(b.N, b.total_bases, b.max_len, b.flags, allowed) || (b.N > 0 && !b.read_offsets) || (b.total_bases > 0 && !b.bases);
}

// an SMEM call's traversal: one of the three, and with GENIE_READS_SPLIT_BREAKS the BWA one
static bool bad_smem_mode(int32_t mode, int32_t flags)
{
    return mode < GENIE_MODE_BWA || mode > GENIE_MODE_RMI || ((flags & GENIE_READS_SPLIT_BREAKS) && mode != GENIE_MODE_BWA);
}

// Reads need their workspace: present, 256-byte aligned and of `need` bytes
static int workspace_args(const CsrBatch &b, int64_t need)
{
    return b.N > 0 && (!b.ws || misaligned(b.ws, 255) || b.ws_bytes < need) ? GENIE_E_CAPACITY : GENIE_OK;
}

static bool bad_contig_count(int64_t n_contigs) { return n_contigs < 1 || n_contigs > 0x7ffffffell; }

int64_t genie_find_smems_long_ex_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags)
{
    if (bad_batch(N, total_bases, max_len, flags, kReadFlags)) return (int64_t)GENIE_E_INVALID;
    return find_smems_long_ex_workspace_bytes(N, total_bases, flags);
}

int genie_find_smems_long_ex(const genie_index *ix, int32_t mode, int32_t flags, const uint8_t *d_bases, const int64_t *d_read_offsets,
                             int64_t N, int64_t total_bases, int64_t max_len, int32_t min_len, int64_t *d_offsets, int32_t *d_rows,
                             int64_t out_cap_rows, int32_t *d_status, void *d_workspace, int64_t workspace_bytes, void *stream)
{
    const CsrBatch b{flags, d_bases, d_read_offsets, N, total_bases, max_len, d_status, d_workspace, workspace_bytes};
    // argument checks first: they need no device image.  Here a missing or misaligned workspace is a bad argument, and only
    // a small one a capacity: the sign of workspace_bytes is not looked at
    if (!ix || bad_batch(b, kReadFlags) || bad_smem_mode(mode, flags) || out_cap_rows < 0 || !d_offsets ||
        (N > 0 && (!d_rows || !d_workspace)) || misaligned(d_rows, 15) || misaligned(d_workspace, 255))
        return GENIE_E_INVALID;
    int rc = workspace_args(b, find_smems_long_ex_workspace_bytes(N, total_bases, flags));
    if (rc || (rc = ready(ix)) || (rc = mode_tables(ix, mode))) return rc;
    return launch_find_smems_long_ex(ix, mode, min_len, b, {d_offsets, d_rows, out_cap_rows, nullptr}, stream);
}

int64_t genie_match_stats_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags)
{
    if (bad_batch(N, total_bases, max_len, flags, kReadFlags)) return (int64_t)GENIE_E_INVALID;
    return match_stats_workspace_bytes(N, total_bases, flags);
}

// genie_match_stats and genie_match_stats_contigs
static bool bad_stats_args(const CsrBatch &b, const int32_t *d_ms, const int32_t *d_lohi)
{
    return bad_batch(b, kReadFlags) || b.ws_bytes < 0 || (b.total_bases > 0 && !d_ms) || misaligned(d_ms, 3) || misaligned(d_lohi, 7);
}

int genie_match_stats(const genie_index *ix, int32_t flags, const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N,
                      int64_t total_bases, int64_t max_len, int32_t *d_ms, int32_t *d_lohi, int32_t *d_status, void *d_workspace,
                      int64_t workspace_bytes, void *stream)
{
    const CsrBatch b{flags, d_bases, d_read_offsets, N, total_bases, max_len, d_status, d_workspace, workspace_bytes};
    // argument checks first: they need no device image
    if (!ix || bad_stats_args(b, d_ms, d_lohi)) return GENIE_E_INVALID;
    int rc = workspace_args(b, match_stats_workspace_bytes(N, total_bases, flags));
    if (rc || (rc = ready(ix))) return rc;
    return launch_match_stats(ix, b, d_ms, d_lohi, stream);
}

int64_t genie_find_mems_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags)
{
    if (bad_batch(N, total_bases, max_len, flags, kReadFlags)) return (int64_t)GENIE_E_INVALID;
    return find_mems_workspace_bytes(N, total_bases, flags);
}

// genie_find_mems and genie_find_mems_contigs: both offset arrays hold N + 1 entries, one at least, and are wanted even
// without reads
static bool bad_mems_args(const CsrBatch &b, int32_t min_len, int32_t max_occ, const CsrRows &out)
{
    return bad_batch(b, kReadFlags) || b.ws_bytes < 0 || out.cap_rows < 0 || min_len < 1 || max_occ < 0 || !out.offsets ||
           !b.read_offsets || misaligned(out.rows, 15) || misaligned(out.offsets, 7) || misaligned(out.totals, 7) ||
           misaligned(b.status, 3);
}

int genie_find_mems(const genie_index *ix, int32_t flags, const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N,
                    int64_t total_bases, int64_t max_len, int32_t min_len, int32_t max_occ, int64_t *d_offsets, int32_t *d_rows,
                    int64_t out_cap_rows, int32_t *d_status, int64_t *d_totals, void *d_workspace, int64_t workspace_bytes,
                    void *stream)
{
    const CsrBatch b{flags, d_bases, d_read_offsets, N, total_bases, max_len, d_status, d_workspace, workspace_bytes};
    const CsrRows out{d_offsets, d_rows, out_cap_rows, d_totals};
    // argument checks first: they need no device image
    if (!ix || bad_mems_args(b, min_len, max_occ, out)) return GENIE_E_INVALID;
    int rc = workspace_args(b, find_mems_workspace_bytes(N, total_bases, flags));
    if (rc || (rc = ready(ix))) return rc;
    return launch_find_mems(ix, b, min_len, max_occ, out, stream);
}

// A contig table as an argument: present, 8-byte aligned, at least one contig and no more than an int counts
static int contig_args(const int64_t *d_contig_offsets, int64_t n_contigs)
{
    if (!d_contig_offsets || n_contigs < 1 || (reinterpret_cast<uintptr_t>(d_contig_offsets) & 7) != 0) return GENIE_E_INVALID;
    return n_contigs > 0x7ffffffell ? GENIE_E_TOO_LONG : GENIE_OK;
}

int genie_contigs_validate(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, void *stream)
{
    if (!ix) return GENIE_E_INVALID;
    int rc = contig_args(d_contig_offsets, n_contigs);
    if (rc || (rc = ready(ix))) return rc;
    return contigs_validate(ix, d_contig_offsets, n_contigs, stream);
}

int64_t genie_find_mems_contigs_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags, int64_t n_contigs)
{
    if (bad_contig_count(n_contigs) || bad_batch(N, total_bases, max_len, flags, kReadFlags)) return (int64_t)GENIE_E_INVALID;
    return find_mems_contigs_workspace_bytes(N, total_bases, flags);
}

// The contig calls: the table's own checks come behind the other arguments' and before the capacity
int genie_find_mems_contigs(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t flags,
                            const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N, int64_t total_bases, int64_t max_len,
                            int32_t min_len, int32_t max_occ, int64_t *d_offsets, int32_t *d_rows, int64_t out_cap_rows,
                            int32_t *d_status, int64_t *d_totals, void *d_workspace, int64_t workspace_bytes, void *stream)
{
    const CsrBatch b{flags, d_bases, d_read_offsets, N, total_bases, max_len, d_status, d_workspace, workspace_bytes};
    const CsrRows out{d_offsets, d_rows, out_cap_rows, d_totals};
    // argument checks first: they need no device image
    if (!ix || bad_mems_args(b, min_len, max_occ, out)) return GENIE_E_INVALID;
    int rc = contig_args(d_contig_offsets, n_contigs);
    if (rc || (rc = workspace_args(b, find_mems_contigs_workspace_bytes(N, total_bases, flags))) || (rc = ready(ix))) return rc;
    return launch_find_mems_contigs(ix, {d_contig_offsets, n_contigs}, b, min_len, max_occ, out, stream);
}

int64_t genie_locate_contigs_tmp_bytes(int64_t S) { return S < 0 ? (int64_t)GENIE_E_INVALID : locate_contigs_tmp_bytes(S); }

int genie_locate_contigs(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, const int32_t *d_rows, int64_t S,
                         int64_t *d_hit_offsets, int32_t *d_hits, int64_t cap_hits, int64_t *d_totals, void *d_tmp, int64_t tmp_bytes,
                         void *stream)
{
    // argument checks first: they need no device image
    if (!ix) return GENIE_E_INVALID;
    if (S < 0 || cap_hits < 0 || tmp_bytes < 0 || !d_hit_offsets || (S > 0 && !d_rows)) return GENIE_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(d_rows) & 15) != 0 || (reinterpret_cast<uintptr_t>(d_hits) & 7) != 0 ||
        (reinterpret_cast<uintptr_t>(d_hit_offsets) & 7) != 0 || (reinterpret_cast<uintptr_t>(d_totals) & 7) != 0)
        return GENIE_E_INVALID;
    int rc = contig_args(d_contig_offsets, n_contigs);
    if (rc) return rc;
    if (S > 0 && (!d_tmp || (reinterpret_cast<uintptr_t>(d_tmp) & 255) != 0 || tmp_bytes < locate_contigs_tmp_bytes(S)))
        return GENIE_E_CAPACITY;
    if ((rc = ready(ix))) return rc;
    return launch_locate_contigs(ix, d_contig_offsets, n_contigs, d_rows, S, d_hit_offsets, d_hits, cap_hits, d_totals, d_tmp, stream);
}

int64_t genie_chain_mems_workspace_bytes(int64_t U, int64_t total_rows, int64_t n_contigs)
{
    if (U < 0 || total_rows < 0 || n_contigs < 0 || n_contigs > 0x7ffffffell) return (int64_t)GENIE_E_INVALID;
    return chain_mems_workspace_bytes(U, total_rows, n_contigs);
}

int genie_chain_mems(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, const int64_t *d_offsets,
                     const int32_t *d_rows, int64_t U, int64_t total_rows, int32_t max_dist, int32_t bandwidth, int32_t gap_cost,
                     int32_t max_pred, int32_t min_score, int64_t *d_chain_offsets, int32_t *d_chains, int64_t cap_chains,
                     int32_t *d_anchor_chain, int32_t *d_anchor_pred, int32_t *d_anchor_score, int64_t *d_totals, void *d_workspace,
                     int64_t workspace_bytes, void *stream)
{
    // argument checks first: they need no device image
    if (!ix || !d_offsets || !d_chain_offsets || (total_rows > 0 && !d_rows)) return GENIE_E_INVALID;
    if (U < 0 || total_rows < 0 || cap_chains < 0 || workspace_bytes < 0) return GENIE_E_INVALID;
    if (max_dist < 1 || max_dist > (1 << 22) || bandwidth < 0 || bandwidth > max_dist || gap_cost < 0 || gap_cost > 255 ||
        max_pred < 0 || min_score < 0)
        return GENIE_E_INVALID;
    if (misaligned(d_offsets, 7) || misaligned(d_rows, 15) || misaligned(d_chain_offsets, 7) || misaligned(d_chains, 15) ||
        misaligned(d_anchor_chain, 3) || misaligned(d_anchor_pred, 3) || misaligned(d_anchor_score, 3) || misaligned(d_totals, 7))
        return GENIE_E_INVALID;
    // the table is optional: null with n_contigs == 0, or a table as every contig call takes it
    if (!d_contig_offsets && n_contigs != 0) return GENIE_E_INVALID;
    if (d_contig_offsets)
        if (int rc = contig_args(d_contig_offsets, n_contigs)) return rc;
    if (U > 0 && (!d_workspace || misaligned(d_workspace, 255) || workspace_bytes < chain_mems_workspace_bytes(U, total_rows, n_contigs)))
        return GENIE_E_CAPACITY;
    if (int rc = ready(ix)) return rc;
    const ChainBatch b{d_offsets, d_rows, U, total_rows, max_dist, bandwidth, gap_cost, max_pred, min_score};
    return launch_chain_mems(ix, {d_contig_offsets, n_contigs}, b, {d_chain_offsets, d_chains, cap_chains, d_totals},
                             {d_anchor_chain, d_anchor_pred, d_anchor_score}, d_workspace, stream);
}

int64_t genie_align_chains_workspace_bytes(int64_t U, int64_t cap_chains)
{
    if (U < 0 || cap_chains < 0) return (int64_t)GENIE_E_INVALID;
    return align_chains_workspace_bytes(U, cap_chains);
}

// The argument checks genie_align_chains and genie_chain_cigars share, in the header's order up to GENIE_E_TOO_LONG
static int align_args(const genie_index *ix, const CsrBatch &b, const int64_t *d_contig_offsets, int64_t n_contigs, const AlignBatch &ab,
                      const AlignParams &p, const int32_t *d_aln, const int64_t *d_totals)
{
    if (!ix || bad_batch(b, kReadFlags) || !ab.offsets || !ab.chain_offsets) return GENIE_E_INVALID;
    if (ab.U < 0 || ab.total_rows < 0 || ab.cap_chains < 0 || b.ws_bytes < 0 || ab.U != b.strand_reads()) return GENIE_E_INVALID;
    if ((ab.total_rows > 0 && (!ab.rows || !ab.anchor_chain || !ab.anchor_pred)) || (ab.cap_chains > 0 && (!ab.chains || !d_aln)))
        return GENIE_E_INVALID;
    if (p.match < 1 || p.match > 64 || p.mismatch < 0 || p.mismatch > 64 || p.gap_open < 0 || p.gap_open > 64 || p.gap_extend < 1 ||
        p.gap_extend > 64 || p.band < 0 || p.band > 511 || p.max_indel < 0 || p.max_indel > GENIE_ALIGN_MAX_DIAGS - 1 - 2 * p.band ||
        p.end_bonus < 0 || p.end_bonus > 32768)
        return GENIE_E_INVALID;
    if (misaligned(b.read_offsets, 7) || misaligned(ab.offsets, 7) || misaligned(ab.rows, 15) || misaligned(ab.chain_offsets, 7) ||
        misaligned(ab.chains, 15) || misaligned(ab.anchor_chain, 3) || misaligned(ab.anchor_pred, 3) || misaligned(d_aln, 15) ||
        misaligned(d_totals, 7))
        return GENIE_E_INVALID;
    // the table is optional: null with n_contigs == 0, or a table as every contig call takes it
    if (!d_contig_offsets && n_contigs != 0) return GENIE_E_INVALID;
    if (d_contig_offsets)
        if (int rc = contig_args(d_contig_offsets, n_contigs)) return rc;
    return GENIE_OK;
}

// every score fits an int with room to spare: the kernels' minus infinity is -2^30
static bool align_too_long(int64_t max_len, const AlignParams &p)
{
    const int64_t worst = std::max<int64_t>(std::max(p.match, p.mismatch), p.gap_open + p.gap_extend);
    return (2 * max_len + p.max_indel + 2 * p.band + 2) * worst + 2 * (int64_t)p.end_bonus >= ((int64_t)1 << 30);
}

int genie_align_chains(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t flags, const uint8_t *d_bases,
                       const int64_t *d_read_offsets, int64_t N, int64_t total_bases, int64_t max_len, const int64_t *d_offsets,
                       const int32_t *d_rows, int64_t U, int64_t total_rows, const int32_t *d_anchor_chain, const int32_t *d_anchor_pred,
                       const int64_t *d_chain_offsets, const int32_t *d_chains, int64_t cap_chains, int32_t match, int32_t mismatch,
                       int32_t gap_open, int32_t gap_extend, int32_t band, int32_t max_indel, int32_t end_bonus, int32_t *d_aln,
                       int64_t *d_totals, void *d_workspace, int64_t workspace_bytes, void *stream)
{
    const CsrBatch b{flags, d_bases, d_read_offsets, N, total_bases, max_len, nullptr, d_workspace, workspace_bytes};
    const AlignBatch ab{d_offsets, d_rows, U, total_rows, d_anchor_chain, d_anchor_pred, d_chain_offsets, d_chains, cap_chains};
    const AlignParams prm{match, mismatch, gap_open, gap_extend, band, max_indel, end_bonus};
    // argument checks first: they need no device image
    if (int rc = align_args(ix, b, d_contig_offsets, n_contigs, ab, prm, d_aln, d_totals)) return rc;
    if (align_too_long(max_len, prm)) return GENIE_E_TOO_LONG;
    if (U > 0 && (!d_workspace || misaligned(d_workspace, 255) || workspace_bytes < align_chains_workspace_bytes(U, cap_chains)))
        return GENIE_E_CAPACITY;
    if (int rc = ready(ix)) return rc;
    return launch_align_chains(ix, {d_contig_offsets, n_contigs}, b, ab, prm, d_aln, d_totals, stream);
}

int64_t genie_chain_cigars_workspace_bytes(int64_t U, int64_t cap_chains, int64_t n_sel, int64_t dir_bytes)
{
    if (U < 0 || cap_chains < 0 || n_sel < 0 || dir_bytes < 0) return (int64_t)GENIE_E_INVALID;
    return chain_cigars_workspace_bytes(U, cap_chains, n_sel, dir_bytes);
}

int genie_chain_cigars(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t flags, const uint8_t *d_bases,
                       const int64_t *d_read_offsets, int64_t N, int64_t total_bases, int64_t max_len, const int64_t *d_offsets,
                       const int32_t *d_rows, int64_t U, int64_t total_rows, const int32_t *d_anchor_chain, const int32_t *d_anchor_pred,
                       const int64_t *d_chain_offsets, const int32_t *d_chains, int64_t cap_chains, int32_t match, int32_t mismatch,
                       int32_t gap_open, int32_t gap_extend, int32_t band, int32_t max_indel, int32_t end_bonus, const int32_t *d_aln,
                       const int64_t *d_sel, int64_t n_sel, int64_t *d_cigar_offsets, uint32_t *d_cigar, int64_t cap_ops, int32_t *d_info,
                       int64_t *d_dir_need, int64_t *d_totals, int64_t dir_bytes, void *d_workspace, int64_t workspace_bytes,
                       void *stream)
{
    const CsrBatch b{flags, d_bases, d_read_offsets, N, total_bases, max_len, nullptr, d_workspace, workspace_bytes};
    const AlignBatch ab{d_offsets, d_rows, U, total_rows, d_anchor_chain, d_anchor_pred, d_chain_offsets, d_chains, cap_chains};
    const AlignParams prm{match, mismatch, gap_open, gap_extend, band, max_indel, end_bonus};
    // argument checks first: they need no device image
    if (int rc = align_args(ix, b, d_contig_offsets, n_contigs, ab, prm, d_aln, d_totals)) return rc;
    if (!d_aln || !d_cigar_offsets || !d_info || n_sel < 0 || cap_ops < 0 || dir_bytes < 0) return GENIE_E_INVALID;
    if (misaligned(d_sel, 7) || misaligned(d_cigar_offsets, 7) || misaligned(d_info, 15) || misaligned(d_cigar, 3) ||
        misaligned(d_dir_need, 7))
        return GENIE_E_INVALID;
    if (align_too_long(max_len, prm)) return GENIE_E_TOO_LONG;
    const int64_t sel = d_sel ? n_sel : cap_chains;
    if ((U > 0 || sel > 0) && (!d_workspace || misaligned(d_workspace, 255) ||
                               workspace_bytes < chain_cigars_workspace_bytes(U, cap_chains, sel, dir_bytes)))
        return GENIE_E_CAPACITY;
    if (int rc = ready(ix)) return rc;
    return launch_chain_cigars(ix, {d_contig_offsets, n_contigs}, b, ab, prm, d_aln,
                               {d_sel, n_sel, d_cigar_offsets, d_cigar, cap_ops, d_info, d_dir_need, d_totals, dir_bytes}, stream);
}

int64_t genie_select_alignments_workspace_bytes(int64_t N, int64_t cap_chains)
{
    if (N < 0 || cap_chains < 0) return (int64_t)GENIE_E_INVALID;
    return select_alignments_workspace_bytes(N, cap_chains);
}

int genie_select_alignments(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t flags,
                            const int64_t *d_read_offsets, int64_t N, const int64_t *d_chain_offsets, int64_t U, const int32_t *d_chains,
                            const int32_t *d_aln, int64_t cap_chains, int32_t mask_level, int32_t pri_ratio, int32_t max_secondary,
                            int32_t min_score, int32_t mapq_full, int32_t *d_class, int64_t *d_sel_offsets, int64_t *d_sel,
                            int32_t *d_records, int64_t cap_sel, int32_t *d_read_counts, int64_t *d_totals, void *d_workspace,
                            int64_t workspace_bytes, void *stream)
{
    // argument checks first: they need no device image
    if (!ix || !d_chain_offsets || !d_sel_offsets || (N > 0 && !d_read_offsets)) return GENIE_E_INVALID;
    if (cap_chains > 0 && (!d_chains || !d_aln || !d_class)) return GENIE_E_INVALID;
    if (d_sel && !d_records) return GENIE_E_INVALID;
    if (N < 0 || U < 0 || cap_chains < 0 || cap_sel < 0 || workspace_bytes < 0 || (flags & ~kReadFlags) != 0) return GENIE_E_INVALID;
    const int32_t S = (flags & GENIE_READS_BOTH_STRANDS) ? 2 : 1;
    if (N > 0x7fffffffffffffffll / S || U != S * N) return GENIE_E_INVALID;
    if (mask_level < 0 || mask_level > 100 || pri_ratio < 0 || pri_ratio > 100 || max_secondary < 0 || max_secondary > (1 << 20) ||
        min_score < 1 || min_score > (1 << 30) || mapq_full < 1 || mapq_full > (1 << 20))
        return GENIE_E_INVALID;
    if (misaligned(d_read_offsets, 7) || misaligned(d_chain_offsets, 7) || misaligned(d_chains, 15) || misaligned(d_aln, 15) ||
        misaligned(d_class, 15) || misaligned(d_sel_offsets, 7) || misaligned(d_sel, 7) || misaligned(d_records, 15) ||
        misaligned(d_read_counts, 15) || misaligned(d_totals, 7))
        return GENIE_E_INVALID;
    // the table is optional: null with n_contigs == 0, or a table as every contig call takes it
    if (!d_contig_offsets && n_contigs != 0) return GENIE_E_INVALID;
    if (d_contig_offsets)
        if (int rc = contig_args(d_contig_offsets, n_contigs)) return rc;
    // reads and chains are named by an int32 in d_class and d_records
    if (N > 0x7fffffffll || cap_chains > 0x7fffffffll) return GENIE_E_TOO_LONG;
    if (U > 0 && (!d_workspace || misaligned(d_workspace, 255) || workspace_bytes < select_alignments_workspace_bytes(N, cap_chains)))
        return GENIE_E_CAPACITY;
    if (int rc = ready(ix)) return rc;
    const SelectBatch b{d_read_offsets, N, S, d_chain_offsets, U, d_chains, d_aln, cap_chains, mask_level, pri_ratio, max_secondary,
                        min_score, mapq_full};
    return launch_select_alignments(ix, {d_contig_offsets, n_contigs}, b,
                                    {d_class, d_sel_offsets, d_sel, d_records, cap_sel, d_read_counts, d_totals}, d_workspace, stream);
}

int64_t genie_pair_alignments_workspace_bytes(int64_t N, int64_t n_records)
{
    if (N < 0 || n_records < 0) return (int64_t)GENIE_E_INVALID;
    return pair_alignments_workspace_bytes(N, n_records);
}

int genie_pair_alignments(const genie_index *ix, int64_t N, const int64_t *d_sel_offsets, const int32_t *d_records, int64_t n_records,
                          const int32_t *d_class, int64_t cap_chains, int32_t orient, int32_t isize_min, int32_t isize_max,
                          int32_t isize_mean, int32_t pen_slope, int32_t pen_max, int32_t pen_unpaired, int32_t mapq_boost,
                          int32_t *d_pairs, int32_t *d_sam, int64_t *d_totals, void *d_workspace, int64_t workspace_bytes, void *stream)
{
    // argument checks first: they need no device image
    if (!ix || !d_sel_offsets || !d_pairs) return GENIE_E_INVALID;
    if (N < 0 || (N & 1) != 0 || n_records < 0 || cap_chains < 0 || workspace_bytes < 0) return GENIE_E_INVALID;
    if (n_records > 0 && (!d_records || !d_sam)) return GENIE_E_INVALID;
    if (cap_chains > 0 && !d_class) return GENIE_E_INVALID;
    const int32_t isize_most = 1 << 30;
    if (orient < 1 || orient > 7 || isize_min < 0 || isize_min > isize_most || isize_max < 0 || isize_max > isize_most ||
        isize_mean < 0 || isize_mean > isize_most || isize_min > isize_max || pen_slope < 0 || pen_slope > 65536 || pen_max < 0 ||
        pen_max > (1 << 20) || pen_unpaired < 0 || pen_unpaired > (1 << 20) || mapq_boost < 0 || mapq_boost > 60)
        return GENIE_E_INVALID;
    if (misaligned(d_records, 15) || misaligned(d_class, 15) || misaligned(d_pairs, 15) || misaligned(d_sam, 15) ||
        misaligned(d_sel_offsets, 7) || misaligned(d_totals, 7))
        return GENIE_E_INVALID;
    // reads and records are named by an int32 in d_pairs and d_sam
    if (N > 0x7fffffffll || n_records > 0x7fffffffll) return GENIE_E_TOO_LONG;
    if (N > 0 && (!d_workspace || misaligned(d_workspace, 255) || workspace_bytes < pair_alignments_workspace_bytes(N, n_records)))
        return GENIE_E_CAPACITY;
    if (int rc = ready(ix)) return rc;
    const PairBatch b{N, d_sel_offsets, d_records, n_records, d_class, cap_chains, orient, isize_min, isize_max, isize_mean,
                      pen_slope, pen_max, pen_unpaired, mapq_boost};
    return launch_pair_alignments(ix, b, {d_pairs, d_sam, d_totals}, d_workspace, stream);
}

int64_t genie_insert_size_stats_workspace_bytes(int64_t N, int32_t max_span)
{
    if (N < 0 || max_span < 1 || max_span > GENIE_WINDOW_MAX / 2) return (int64_t)GENIE_E_INVALID;
    return insert_size_stats_workspace_bytes(N, max_span);
}

int genie_insert_size_stats(const genie_index *ix, int64_t N, const int64_t *d_sel_offsets, const int32_t *d_records, int64_t n_records,
                            int32_t min_mapq, int32_t max_span, int32_t min_samples, int64_t *d_stats, int32_t *d_samples,
                            int64_t *d_totals, void *d_workspace, int64_t workspace_bytes, void *stream)
{
    // argument checks first: they need no device image
    if (!ix || !d_sel_offsets || !d_stats) return GENIE_E_INVALID;
    if (N < 0 || (N & 1) != 0 || n_records < 0 || workspace_bytes < 0) return GENIE_E_INVALID;
    if (n_records > 0 && !d_records) return GENIE_E_INVALID;
    if (min_mapq < 0 || min_mapq > 60 || max_span < 1 || max_span > GENIE_WINDOW_MAX / 2 || min_samples < 1 || min_samples > (1 << 30))
        return GENIE_E_INVALID;
    if (misaligned(d_records, 15) || misaligned(d_sel_offsets, 7) || misaligned(d_stats, 7) || misaligned(d_samples, 7) ||
        misaligned(d_totals, 7))
        return GENIE_E_INVALID;
    // reads and records are named by an int32, and a bin's count stays below 2^30
    if (N > 0x7fffffffll || n_records > 0x7fffffffll) return GENIE_E_TOO_LONG;
    if (N > 0 && (!d_workspace || misaligned(d_workspace, 255) || workspace_bytes < insert_size_stats_workspace_bytes(N, max_span)))
        return GENIE_E_CAPACITY;
    if (int rc = ready(ix)) return rc;
    const IsizeBatch b{N, d_sel_offsets, d_records, n_records, min_mapq, max_span, min_samples};
    return launch_insert_size_stats(ix, b, {d_stats, d_samples, d_totals}, d_workspace, stream);
}

int64_t genie_rescue_windows_workspace_bytes(int64_t N)
{
    if (N < 0) return (int64_t)GENIE_E_INVALID;
    return rescue_windows_workspace_bytes(N);
}

int genie_rescue_windows(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, const int64_t *d_read_offsets,
                         int64_t N, const int64_t *d_sel_offsets, const int32_t *d_records, int64_t n_records, const int32_t *d_pairs,
                         int32_t orient, int32_t isize_max, int32_t min_anchor_score, int32_t *d_windows, int64_t *d_totals,
                         void *d_workspace, int64_t workspace_bytes, void *stream)
{
    // argument checks first: they need no device image
    if (!ix || !d_sel_offsets) return GENIE_E_INVALID;
    if (N < 0 || (N & 1) != 0 || n_records < 0 || workspace_bytes < 0) return GENIE_E_INVALID;
    if (N > 0 && (!d_read_offsets || !d_pairs || !d_windows)) return GENIE_E_INVALID;
    if (n_records > 0 && !d_records) return GENIE_E_INVALID;
    if (orient < 1 || orient > 7 || isize_max < 1 || isize_max > GENIE_WINDOW_MAX / 2 || min_anchor_score < 0 ||
        min_anchor_score > (1 << 30))
        return GENIE_E_INVALID;
    if (misaligned(d_records, 15) || misaligned(d_pairs, 15) || misaligned(d_read_offsets, 7) || misaligned(d_sel_offsets, 7) ||
        misaligned(d_windows, 7) || misaligned(d_totals, 7))
        return GENIE_E_INVALID;
    // the table is optional: null with n_contigs == 0, or a table as every contig call takes it
    if (!d_contig_offsets && n_contigs != 0) return GENIE_E_INVALID;
    if (d_contig_offsets)
        if (int rc = contig_args(d_contig_offsets, n_contigs)) return rc;
    // reads and records are named by an int32 in d_pairs
    if (N > 0x7fffffffll || n_records > 0x7fffffffll) return GENIE_E_TOO_LONG;
    if (N > 0 && (!d_workspace || misaligned(d_workspace, 255) || workspace_bytes < rescue_windows_workspace_bytes(N)))
        return GENIE_E_CAPACITY;
    if (int rc = ready(ix)) return rc;
    const RescueBatch b{N, d_read_offsets, d_sel_offsets, d_records, n_records, d_pairs, orient, isize_max, min_anchor_score};
    return launch_rescue_windows(ix, {d_contig_offsets, n_contigs}, b, d_windows, d_totals, d_workspace, stream);
}

int64_t genie_window_mems_workspace_bytes(int64_t U)
{
    if (U < 0) return (int64_t)GENIE_E_INVALID;
    return window_mems_workspace_bytes(U);
}

int genie_window_mems(const genie_index *ix, int32_t flags, const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N,
                      int64_t total_bases, int64_t max_len, int64_t U, const int32_t *d_windows, int32_t min_len,
                      const int64_t *d_in_offsets, const int32_t *d_in_rows, int64_t in_total_rows, int64_t *d_offsets, int32_t *d_rows,
                      int64_t out_cap_rows, int32_t *d_status, int64_t *d_totals, void *d_workspace, int64_t workspace_bytes,
                      void *stream)
{
    const CsrBatch b{flags, d_bases, d_read_offsets, N, total_bases, max_len, d_status, d_workspace, workspace_bytes};
    // argument checks first: they need no device image
    if (!ix || bad_batch(b, kReadFlags) || !d_offsets || !d_read_offsets) return GENIE_E_INVALID;
    if (U < 0 || N > 0x7fffffffffffffffll / b.strands() || U != b.strand_reads() || out_cap_rows < 0 || in_total_rows < 0 ||
        workspace_bytes < 0 || min_len < 1)
        return GENIE_E_INVALID;
    if ((U > 0 && !d_windows) || (d_in_offsets && in_total_rows > 0 && !d_in_rows)) return GENIE_E_INVALID;
    if (misaligned(d_rows, 15) || misaligned(d_in_rows, 15) || misaligned(d_offsets, 7) || misaligned(d_in_offsets, 7) ||
        misaligned(d_read_offsets, 7) || misaligned(d_windows, 7) || misaligned(d_totals, 7) || misaligned(d_status, 3))
        return GENIE_E_INVALID;
    // units are named by an int32 in the list of the units to search
    if (U > 0x7fffffffll) return GENIE_E_TOO_LONG;
    if (U > 0 && (!d_workspace || misaligned(d_workspace, 255) || workspace_bytes < window_mems_workspace_bytes(U)))
        return GENIE_E_CAPACITY;
    if (int rc = ready(ix)) return rc;
    const WindowBatch wb{U, d_windows, min_len, d_in_offsets, d_in_rows, in_total_rows};
    return launch_window_mems(ix, b, wb, {d_offsets, d_rows, out_cap_rows, d_totals}, stream);
}

int64_t genie_sam_text_workspace_bytes(int64_t N, int64_t n_records)
{
    if (N < 0 || n_records < 0) return (int64_t)GENIE_E_INVALID;
    return sam_text_workspace_bytes(N, n_records);
}

// the checks that genie_sam_text and genie_bam_records share, in the header's order; `out` holds the call's line or record
// offsets and its text or data, workspace_needed its workspace function, called only with sizes that passed the checks
// before it.  GENIE_OK: the device check has passed too.
static int sam_args(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, const SamBatch &b, const SamTextOut &out,
                    const void *d_workspace, int64_t workspace_bytes, int64_t (*workspace_needed)(int64_t, int64_t))
{
    // argument checks first: they need no device image
    if (!ix || !b.read_offsets || !b.sel_offsets || !b.name_offsets || !b.contig_name_offsets || !out.line_offsets) return GENIE_E_INVALID;
    if (b.N < 0 || b.total_bases < 0 || b.n_records < 0 || b.n_ops < 0 || b.name_bytes < 0 || b.contig_name_bytes < 0 || out.cap_text < 0 ||
        workspace_bytes < 0)
        return GENIE_E_INVALID;
    if (b.sam && (b.N & 1) != 0) return GENIE_E_INVALID;
    if ((b.tags & ~(GENIE_SAM_NM | GENIE_SAM_AS | GENIE_SAM_MD | GENIE_SAM_MC | GENIE_SAM_MQ)) != 0 || (b.flags & ~GENIE_SAM_NO_SEQ) != 0)
        return GENIE_E_INVALID;
    if ((b.total_bases > 0 && !b.bases) || (b.name_bytes > 0 && !b.names) || (b.contig_name_bytes > 0 && !b.contig_names) ||
        (b.n_ops > 0 && !b.cigar))
        return GENIE_E_INVALID;
    if (b.n_records > 0 && (!b.records || !b.info || !b.cigar_offsets)) return GENIE_E_INVALID;
    if (misaligned(b.records, 15) || misaligned(b.sam, 15) || misaligned(b.info, 15) || misaligned(b.read_offsets, 7) ||
        misaligned(b.sel_offsets, 7) || misaligned(b.cigar_offsets, 7) || misaligned(b.name_offsets, 7) ||
        misaligned(b.contig_name_offsets, 7) || misaligned(out.line_offsets, 7) || misaligned(out.totals, 7) || misaligned(b.cigar, 3))
        return GENIE_E_INVALID;
    // the table is optional: null with n_contigs == 0, or a table as every contig call takes it
    if (!d_contig_offsets && n_contigs != 0) return GENIE_E_INVALID;
    if (d_contig_offsets)
        if (int rc = contig_args(d_contig_offsets, n_contigs)) return rc;
    // reads and records are named by an int32 in the table of lines
    if (b.N > 0x7fffffffll || b.n_records > 0x7fffffffll) return GENIE_E_TOO_LONG;
    if (b.N > 0 && (!d_workspace || misaligned(d_workspace, 255) || workspace_bytes < workspace_needed(b.N, b.n_records)))
        return GENIE_E_CAPACITY;
    return ready(ix);
}

int genie_sam_text(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, const uint8_t *d_bases,
                   const int64_t *d_read_offsets, int64_t N, int64_t total_bases, const uint8_t *d_quals, const int64_t *d_sel_offsets,
                   const int32_t *d_records, int64_t n_records, const int32_t *d_sam, const int32_t *d_info,
                   const int64_t *d_cigar_offsets, const uint32_t *d_cigar, int64_t n_ops, const uint8_t *d_names,
                   const int64_t *d_name_offsets, int64_t name_bytes, const uint8_t *d_contig_names,
                   const int64_t *d_contig_name_offsets, int64_t contig_name_bytes, int32_t tags, int32_t flags,
                   int64_t *d_line_offsets, uint8_t *d_text, int64_t cap_text, int64_t *d_totals, void *d_workspace,
                   int64_t workspace_bytes, void *stream)
{
    const SamBatch b{d_bases, d_read_offsets, N, total_bases, d_quals, d_sel_offsets, d_records, n_records, d_sam, d_info,
                     d_cigar_offsets, d_cigar, n_ops, d_names, d_name_offsets, name_bytes, d_contig_names, d_contig_name_offsets,
                     contig_name_bytes, tags, flags};
    const SamTextOut out{d_line_offsets, d_text, cap_text, d_totals};
    if (int rc = sam_args(ix, d_contig_offsets, n_contigs, b, out, d_workspace, workspace_bytes, sam_text_workspace_bytes)) return rc;
    return launch_sam_text(ix, {d_contig_offsets, n_contigs}, b, out, d_workspace, stream);
}

int64_t genie_bam_records_workspace_bytes(int64_t N, int64_t n_records)
{
    if (N < 0 || n_records < 0) return (int64_t)GENIE_E_INVALID;
    return bam_records_workspace_bytes(N, n_records);
}

int genie_bam_records(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, const uint8_t *d_bases,
                      const int64_t *d_read_offsets, int64_t N, int64_t total_bases, const uint8_t *d_quals, const int64_t *d_sel_offsets,
                      const int32_t *d_records, int64_t n_records, const int32_t *d_sam, const int32_t *d_info,
                      const int64_t *d_cigar_offsets, const uint32_t *d_cigar, int64_t n_ops, const uint8_t *d_names,
                      const int64_t *d_name_offsets, int64_t name_bytes, const uint8_t *d_contig_names,
                      const int64_t *d_contig_name_offsets, int64_t contig_name_bytes, int32_t tags, int32_t flags,
                      int64_t *d_record_offsets, uint8_t *d_data, int64_t cap_data, int64_t *d_totals, void *d_workspace,
                      int64_t workspace_bytes, void *stream)
{
    const SamBatch b{d_bases, d_read_offsets, N, total_bases, d_quals, d_sel_offsets, d_records, n_records, d_sam, d_info,
                     d_cigar_offsets, d_cigar, n_ops, d_names, d_name_offsets, name_bytes, d_contig_names, d_contig_name_offsets,
                     contig_name_bytes, tags, flags};
    const SamTextOut out{d_record_offsets, d_data, cap_data, d_totals};
    if (int rc = sam_args(ix, d_contig_offsets, n_contigs, b, out, d_workspace, workspace_bytes, bam_records_workspace_bytes)) return rc;
    return launch_bam_records(ix, {d_contig_offsets, n_contigs}, b, out, d_workspace, stream);
}

int genie_contig_coords(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, const int32_t *d_pos, int32_t stride,
                        int64_t count, int32_t *d_out, void *stream)
{
    // argument checks first: they need no device image
    if (!ix) return GENIE_E_INVALID;
    if (count < 0 || stride < 1 || (count > 0 && (!d_pos || !d_out))) return GENIE_E_INVALID;
    if (((reinterpret_cast<uintptr_t>(d_pos) | reinterpret_cast<uintptr_t>(d_out)) & 3) != 0) return GENIE_E_INVALID;
    int rc = contig_args(d_contig_offsets, n_contigs);
    if (rc || (rc = ready(ix))) return rc;
    return launch_contig_coords(ix, d_contig_offsets, n_contigs, d_pos, stride, count, d_out, stream);
}

int64_t genie_match_stats_contigs_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags, int64_t n_contigs)
{
    if (bad_contig_count(n_contigs) || bad_batch(N, total_bases, max_len, flags, kReadFlags)) return (int64_t)GENIE_E_INVALID;
    return match_stats_contigs_workspace_bytes(N, total_bases, flags);
}

int genie_match_stats_contigs(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t flags,
                              const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N, int64_t total_bases, int64_t max_len,
                              int32_t *d_ms, int32_t *d_lohi, int32_t *d_status, int64_t *d_totals, void *d_workspace,
                              int64_t workspace_bytes, void *stream)
{
    const CsrBatch b{flags, d_bases, d_read_offsets, N, total_bases, max_len, d_status, d_workspace, workspace_bytes};
    // argument checks first: they need no device image
    if (!ix || bad_stats_args(b, d_ms, d_lohi) || misaligned(d_totals, 7)) return GENIE_E_INVALID;
    int rc = contig_args(d_contig_offsets, n_contigs);
    if (rc || (rc = workspace_args(b, match_stats_contigs_workspace_bytes(N, total_bases, flags))) || (rc = ready(ix))) return rc;
    return launch_match_stats_contigs(ix, {d_contig_offsets, n_contigs}, b, d_ms, d_lohi, d_totals, stream);
}

int64_t genie_find_smems_contigs_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags, int64_t n_contigs)
{
    if (bad_contig_count(n_contigs) || bad_batch(N, total_bases, max_len, flags, kReadFlags)) return (int64_t)GENIE_E_INVALID;
    return find_smems_contigs_workspace_bytes(N, total_bases, flags);
}

int genie_find_smems_contigs(const genie_index *ix, const int64_t *d_contig_offsets, int64_t n_contigs, int32_t mode, int32_t flags,
                             const uint8_t *d_bases, const int64_t *d_read_offsets, int64_t N, int64_t total_bases, int64_t max_len,
                             int32_t min_len, int64_t *d_offsets, int32_t *d_rows, int64_t out_cap_rows, int32_t *d_status,
                             int64_t *d_totals, void *d_workspace, int64_t workspace_bytes, void *stream)
{
    const CsrBatch b{flags, d_bases, d_read_offsets, N, total_bases, max_len, d_status, d_workspace, workspace_bytes};
    // argument checks first: they need no device image
    if (!ix || bad_batch(b, kReadFlags) || bad_smem_mode(mode, flags) || workspace_bytes < 0 || out_cap_rows < 0 || !d_offsets ||
        (N > 0 && !d_rows) || misaligned(d_rows, 15) || misaligned(d_totals, 7))
        return GENIE_E_INVALID;
    int rc = contig_args(d_contig_offsets, n_contigs);
    if (rc || (rc = workspace_args(b, find_smems_contigs_workspace_bytes(N, total_bases, flags))) || (rc = ready(ix)) ||
        (rc = mode_tables(ix, mode)))
        return rc;
    return launch_find_smems_contigs(ix, {d_contig_offsets, n_contigs}, mode, min_len, b, {d_offsets, d_rows, out_cap_rows, d_totals}, stream);
}

int64_t genie_match_stats_min_occ_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags)
{
    if (bad_batch(N, total_bases, max_len, flags, kReadFlags)) return (int64_t)GENIE_E_INVALID;
    return match_stats_min_occ_workspace_bytes(N, total_bases, flags);
}

int genie_match_stats_min_occ(const genie_index *ix, int32_t flags, int32_t min_occ, const uint8_t *d_bases, const int64_t *d_read_offsets,
                              int64_t N, int64_t total_bases, int64_t max_len, int32_t *d_ms, int32_t *d_lohi, int32_t *d_status,
                              int64_t *d_totals, void *d_workspace, int64_t workspace_bytes, void *stream)
{
    const CsrBatch b{flags, d_bases, d_read_offsets, N, total_bases, max_len, d_status, d_workspace, workspace_bytes};
    // argument checks first: they need no device image
    if (!ix || bad_stats_args(b, d_ms, d_lohi) || min_occ < 1 || misaligned(d_totals, 7)) return GENIE_E_INVALID;
    int rc = workspace_args(b, match_stats_min_occ_workspace_bytes(N, total_bases, flags));
    if (rc || (rc = ready(ix))) return rc;
    return launch_match_stats_min_occ(ix, min_occ, b, d_ms, d_lohi, d_totals, stream);
}

int64_t genie_find_smems_min_occ_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags)
{
    if (bad_batch(N, total_bases, max_len, flags, kReadFlags)) return (int64_t)GENIE_E_INVALID;
    return find_smems_min_occ_workspace_bytes(N, total_bases, flags);
}

int genie_find_smems_min_occ(const genie_index *ix, int32_t mode, int32_t flags, const uint8_t *d_bases, const int64_t *d_read_offsets,
                             int64_t N, int64_t total_bases, int64_t max_len, int32_t min_len, int32_t min_occ, int64_t *d_offsets,
                             int32_t *d_rows, int64_t out_cap_rows, int32_t *d_status, int64_t *d_totals, void *d_workspace,
                             int64_t workspace_bytes, void *stream)
{
    const CsrBatch b{flags, d_bases, d_read_offsets, N, total_bases, max_len, d_status, d_workspace, workspace_bytes};
    // the checks of genie_find_smems_long_ex, in its order, then this call's own
    if (!ix || bad_batch(b, kReadFlags) || bad_smem_mode(mode, flags) || out_cap_rows < 0 || !d_offsets ||
        (N > 0 && (!d_rows || !d_workspace)) || misaligned(d_rows, 15) || misaligned(d_workspace, 255) || min_occ < 1 ||
        misaligned(d_totals, 7))
        return GENIE_E_INVALID;
    int rc = workspace_args(b, find_smems_min_occ_workspace_bytes(N, total_bases, flags));
    if (rc || (rc = ready(ix)) || (rc = mode_tables(ix, mode))) return rc;
    return launch_find_smems_min_occ(ix, mode, min_len, min_occ, b, {d_offsets, d_rows, out_cap_rows, d_totals}, stream);
}

int64_t genie_exact_match_workspace_bytes(int64_t N, int64_t total_bases, int64_t max_len, int32_t flags)
{
    if (bad_batch(N, total_bases, max_len, flags, GENIE_READS_BOTH_STRANDS)) return (int64_t)GENIE_E_INVALID;
    return exact_match_workspace_bytes(N, total_bases, flags);
}

int genie_exact_match(const genie_index *ix, int32_t flags, const uint8_t *d_bases, const int64_t *d_pat_offsets, int64_t N,
                      int64_t total_bases, int64_t max_len, int32_t *d_lohi, int32_t *d_counts, int32_t *d_status, void *d_workspace,
                      int64_t workspace_bytes, void *stream)
{
    const CsrBatch b{flags, d_bases, d_pat_offsets, N, total_bases, max_len, d_status, d_workspace, workspace_bytes};
    // argument checks first: they need no device image.  GENIE_READS_SPLIT_BREAKS is refused too: a pattern with a break
    // has no interval
    if (!ix || bad_batch(b, GENIE_READS_BOTH_STRANDS) || workspace_bytes < 0 || (N > 0 && !d_lohi) || misaligned(d_lohi, 7) ||
        misaligned(d_counts, 3) || misaligned(d_status, 3))
        return GENIE_E_INVALID;
    int rc = workspace_args(b, exact_match_workspace_bytes(N, total_bases, flags));
    if (rc || (rc = ready(ix))) return rc;
    return launch_exact_match(ix, b, d_lohi, d_counts, stream);
}

int64_t genie_reads_from_text_tmp_bytes(int64_t text_bytes, int64_t cap_reads)
{
    if (text_bytes < 0 || cap_reads < 0) return (int64_t)GENIE_E_INVALID;
    return reads_from_text_tmp_bytes(text_bytes, cap_reads);
}

int genie_reads_from_text(const uint8_t *d_text, int64_t text_bytes, int32_t format, int32_t flags, const uint8_t *code_of_byte,
                          uint8_t *d_bases, int64_t cap_bases, int64_t *d_read_offsets, int64_t cap_reads, int64_t *out5,
                          void *d_tmp, int64_t tmp_bytes, void *stream)
{
    // argument checks first: they need no device
    if (text_bytes < 0 || cap_bases < 0 || cap_reads < 0 || tmp_bytes < 0 || !code_of_byte || !out5 || (text_bytes > 0 && !d_text))
        return GENIE_E_INVALID;
    if ((format != GENIE_TEXT_LINES && format != GENIE_TEXT_FASTQ) || (flags & ~GENIE_TEXT_PARTIAL)) return GENIE_E_INVALID;
    if ((d_bases == nullptr) != (d_read_offsets == nullptr)) return GENIE_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(d_read_offsets) & 7) != 0) return GENIE_E_INVALID;
    if (!d_tmp || (reinterpret_cast<uintptr_t>(d_tmp) & 255) != 0 || tmp_bytes < reads_from_text_tmp_bytes(text_bytes, cap_reads))
        return GENIE_E_CAPACITY;
    return launch_reads_from_text(d_text, text_bytes, format, flags, code_of_byte, d_bases, cap_bases, d_read_offsets, cap_reads, out5,
                                  d_tmp, stream);
}

int64_t genie_reads_from_fasta_tmp_bytes(int64_t text_bytes, int64_t cap_reads)
{
    if (text_bytes < 0 || cap_reads < 0) return (int64_t)GENIE_E_INVALID;
    return reads_from_fasta_tmp_bytes(text_bytes, cap_reads);
}

int genie_reads_from_fasta(const uint8_t *d_text, int64_t text_bytes, int32_t flags, const uint8_t *code_of_byte, uint8_t *d_bases,
                           int64_t cap_bases, int64_t *d_read_offsets, int64_t *d_record_starts, int64_t cap_reads, int64_t *out5,
                           void *d_tmp, int64_t tmp_bytes, void *stream)
{
    // argument checks first: they need no device
    if (text_bytes < 0 || cap_bases < 0 || cap_reads < 0 || tmp_bytes < 0 || !code_of_byte || !out5 || (text_bytes > 0 && !d_text))
        return GENIE_E_INVALID;
    if (flags & ~GENIE_TEXT_PARTIAL) return GENIE_E_INVALID;
    if ((d_bases == nullptr) != (d_read_offsets == nullptr) || (!d_read_offsets && d_record_starts)) return GENIE_E_INVALID;
    if (((reinterpret_cast<uintptr_t>(d_read_offsets) | reinterpret_cast<uintptr_t>(d_record_starts)) & 7) != 0) return GENIE_E_INVALID;
    if (!d_tmp || (reinterpret_cast<uintptr_t>(d_tmp) & 255) != 0 || tmp_bytes < reads_from_fasta_tmp_bytes(text_bytes, cap_reads))
        return GENIE_E_CAPACITY;
    return launch_reads_from_fasta(d_text, text_bytes, flags, code_of_byte, d_bases, cap_bases, d_read_offsets, d_record_starts, cap_reads,
                                   out5, d_tmp, stream);
}

int64_t genie_reference_segments_tmp_bytes(int64_t n_given, int64_t n_records)
{
    if (n_given < 0 || n_records < 0) return (int64_t)GENIE_E_INVALID;
    return reference_segments_tmp_bytes(n_given, n_records);
}

int genie_reference_segments(const uint8_t *d_codes, int64_t n_given, const int64_t *d_record_offsets, int64_t n_records,
                             uint8_t *d_bases, int64_t cap_bases, int64_t *d_seg_offsets, int32_t *d_seg_record, int64_t *d_seg_origin,
                             int64_t cap_segs, int64_t *out4, void *d_tmp, int64_t tmp_bytes, void *stream)
{
    // argument checks first: they need no device
    if (n_given < 0 || tmp_bytes < 0 || n_records < 1 || !out4 || (n_given > 0 && !d_codes)) return GENIE_E_INVALID;
    if (!d_record_offsets && n_records != 1) return GENIE_E_INVALID;
    const int outputs = (d_bases != nullptr) + (d_seg_offsets != nullptr) + (d_seg_record != nullptr) + (d_seg_origin != nullptr);
    if (outputs != 0 && outputs != 4) return GENIE_E_INVALID;
    if (outputs && (cap_bases < 0 || cap_segs < 0)) return GENIE_E_INVALID;      // the sizing call does not look at them
    if (((reinterpret_cast<uintptr_t>(d_record_offsets) | reinterpret_cast<uintptr_t>(d_seg_offsets) |
          reinterpret_cast<uintptr_t>(d_seg_origin)) & 7) != 0 || (reinterpret_cast<uintptr_t>(d_seg_record) & 3) != 0)
        return GENIE_E_INVALID;
    if (n_records > 0x7fffffffll) return GENIE_E_TOO_LONG;             // d_seg_record is int32
    if (!d_tmp || (reinterpret_cast<uintptr_t>(d_tmp) & 255) != 0 || tmp_bytes < reference_segments_tmp_bytes(n_given, n_records))
        return GENIE_E_CAPACITY;
    return launch_reference_segments(d_codes, n_given, d_record_offsets, n_records, d_bases, cap_bases, d_seg_offsets, d_seg_record,
                                     d_seg_origin, cap_segs, out4, d_tmp, stream);
}

int genie_segment_coords(const genie_index *ix, const int64_t *d_seg_offsets, const int32_t *d_seg_record, const int64_t *d_seg_origin,
                         int64_t n_segs, int32_t form, const int32_t *d_in, int32_t stride, int64_t count, int64_t *d_out, void *stream)
{
    // argument checks first: they need no device image
    if (!ix) return GENIE_E_INVALID;
    if (form != GENIE_SEG_POSITIONS && form != GENIE_SEG_HITS) return GENIE_E_INVALID;
    if (count < 0 || stride < (form == GENIE_SEG_HITS ? 2 : 1) || (count > 0 && (!d_in || !d_out))) return GENIE_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(d_in) & 3) != 0 || (reinterpret_cast<uintptr_t>(d_out) & 15) != 0) return GENIE_E_INVALID;
    if (!d_seg_record || !d_seg_origin || (reinterpret_cast<uintptr_t>(d_seg_record) & 3) != 0 ||
        (reinterpret_cast<uintptr_t>(d_seg_origin) & 7) != 0)
        return GENIE_E_INVALID;
    int rc = contig_args(d_seg_offsets, n_segs);
    if (rc || (rc = ready(ix))) return rc;
    return launch_segment_coords(ix, d_seg_offsets, d_seg_record, d_seg_origin, n_segs, form, d_in, stride, count, d_out, stream);
}

static int find_smems_packed_any(const genie_index *ix, int32_t mode, const uint8_t *d_reads2bit, const int32_t *d_lens, int64_t N,
                                 int32_t stride_bytes, int32_t fixed_len, int32_t min_len, uint8_t *d_counts8, uint8_t *d_status8,
                                 void *d_rows, int64_t out_cap_rows, int64_t *d_totals, int64_t *d_escapes, int64_t cap_escapes,
                                 void *d_workspace, int64_t workspace_bytes, void *stream, int row_bytes)
{
    int rc = ready(ix);
    if (rc) return rc;
    if (N < 0 || stride_bytes < 0 || fixed_len < 0 || out_cap_rows < 0 || cap_escapes < 0 || !d_totals ||
        (N > 0 && (!d_reads2bit || !d_rows || !d_counts8 || !d_status8)) || (cap_escapes > 0 && !d_escapes))
        return GENIE_E_INVALID;
    if (mode < GENIE_MODE_BWA || mode > GENIE_MODE_RMI) return GENIE_E_INVALID;
    if (fixed_len > 255) return GENIE_E_TOO_LONG;                       // start / end are bytes in the compact rows
    if (row_bytes == 6 && (int64_t)ix->dev.n + 1 >= (1ll << 24)) return GENIE_E_TOO_LONG;       // lo is 24 bits in the 6-byte rows
    if ((stride_bytes & 3) != 0 || stride_bytes < 4 * ((fixed_len + 15) / 16)) return GENIE_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(d_reads2bit) & 3) != 0 || (reinterpret_cast<uintptr_t>(d_rows) & (row_bytes == 6 ? 1 : 7)) != 0 ||
        (reinterpret_cast<uintptr_t>(d_totals) & 7) != 0)
        return GENIE_E_INVALID;
    if ((rc = mode_tables(ix, mode))) return rc;
    return launch_find_smems_packed(ix, mode, {d_reads2bit, d_lens, N, stride_bytes, fixed_len, min_len, nullptr, d_workspace, workspace_bytes},
                                    d_counts8, d_status8, d_rows, out_cap_rows, d_totals, d_escapes, cap_escapes, stream, row_bytes);
}

int genie_find_smems_packed(const genie_index *ix, int32_t mode, const uint8_t *d_reads2bit, const int32_t *d_lens, int64_t N,
                            int32_t stride_bytes, int32_t fixed_len, int32_t min_len, uint8_t *d_counts8, uint8_t *d_status8,
                            void *d_rows8, int64_t out_cap_rows, int64_t *d_totals, int64_t *d_escapes, int64_t cap_escapes,
                            void *d_workspace, int64_t workspace_bytes, void *stream)
{
    return find_smems_packed_any(ix, mode, d_reads2bit, d_lens, N, stride_bytes, fixed_len, min_len, d_counts8, d_status8, d_rows8,
                                 out_cap_rows, d_totals, d_escapes, cap_escapes, d_workspace, workspace_bytes, stream, 8);
}

int genie_find_smems_packed6(const genie_index *ix, int32_t mode, const uint8_t *d_reads2bit, const int32_t *d_lens, int64_t N,
                             int32_t stride_bytes, int32_t fixed_len, int32_t min_len, uint8_t *d_counts8, uint8_t *d_status8,
                             void *d_rows6, int64_t out_cap_rows, int64_t *d_totals, int64_t *d_escapes, int64_t cap_escapes,
                             void *d_workspace, int64_t workspace_bytes, void *stream)
{
    return find_smems_packed_any(ix, mode, d_reads2bit, d_lens, N, stride_bytes, fixed_len, min_len, d_counts8, d_status8, d_rows6,
                                 out_cap_rows, d_totals, d_escapes, cap_escapes, d_workspace, workspace_bytes, stream, 6);
}

int64_t genie_find_smems_workspace_bytes(int64_t N, int32_t max_len)
{
    if (N < 0 || max_len < 0) return (int64_t)GENIE_E_INVALID;
    return find_smems_workspace_bytes(N, max_len);
}

int genie_find_smems_workspace_rows(int32_t max_len, int32_t *row_bytes4)
{
    if (max_len < 0 || max_len > GENIE_MAX_READ_LEN || !row_bytes4) return GENIE_E_INVALID;
    find_smems_workspace_rows(max_len, row_bytes4);
    return GENIE_OK;
}

int64_t genie_compact_tmp_bytes(int64_t N) { return N < 0 ? (int64_t)GENIE_E_INVALID : compact_tmp_bytes(N); }

int genie_compact_smems(const int32_t *d_counts, const int32_t *d_slots, int64_t N, int32_t cap,
                        int64_t *d_offsets, int32_t *d_out, int64_t out_cap_rows, void *d_tmp, void *stream)
{
    if (N < 0 || cap < 1 || !d_offsets || !d_tmp || (N > 0 && (!d_counts || !d_slots))) return GENIE_E_INVALID;
    return launch_compact(d_counts, d_slots, N, cap, d_offsets, d_out, out_cap_rows, d_tmp, stream);
}

int64_t genie_locate_tmp_bytes(int64_t S) { return S < 0 ? 0 : locate_tmp_bytes(S); }

int genie_locate(const genie_index *ix, const int32_t *d_lohi, int32_t stride, int64_t S, int64_t *d_pos_offsets,
                 int32_t *d_positions, int64_t cap_positions, void *d_tmp, int64_t tmp_bytes, void *stream)
{
    int rc = ready(ix);
    if (rc) return rc;
    if (S < 0 || stride < 2 || !d_pos_offsets || cap_positions < 0 || (S > 0 && !d_lohi) ||
        (cap_positions > 0 && !d_positions))
        return GENIE_E_INVALID;
    return launch_locate(ix, d_lohi, stride, S, d_pos_offsets, d_positions, cap_positions, d_tmp, tmp_bytes, stream);
}

int genie_launch_info(const genie_index *ix, int32_t mode, int32_t max_len, int32_t *grid, int32_t *block,
                      int32_t *lds_bytes)
{
    int rc = ready(ix);
    if (rc) return rc;
    return find_smems_geometry(ix, mode, max_len, grid, block, lds_bytes);
}

int genie_search_kernel_name(const genie_index *ix, int32_t mode, int32_t max_len, char *buf, int32_t cap)
{
    int rc = ready(ix);
    if (rc) return rc;
    if (mode < GENIE_MODE_BWA || mode > GENIE_MODE_RMI) return GENIE_E_INVALID;
    return search_kernel_name(ix, mode, max_len, buf, cap);
}

int genie_index_set_option(genie_index *ix, int32_t option, int32_t value)
{
    if (!ix) return GENIE_E_INVALID;
    switch (option) {
    case GENIE_OPT_SEARCH_ALL: ix->opt_search_all = value != 0; return GENIE_OK;
    case GENIE_OPT_GROUP_POSITIONS: ix->opt_group_positions = value > 0 ? value : 0; return GENIE_OK;
    case GENIE_OPT_SEARCH_ONLY: ix->opt_search_only = value != 0; if (!value) ix->opt_debug = 0; return GENIE_OK;
    case GENIE_OPT_SCHEDULING: ix->opt_scheduling = value & 15; return GENIE_OK;
    case GENIE_OPT_SEARCH_STAGES_OFF: ix->opt_debug = ix->opt_search_only ? (value & 63) : 0; return GENIE_OK;
    case GENIE_OPT_SEARCH_BLOCKS_PER_CU: ix->opt_search_blocks_per_cu = value > 0 ? value : 0; return GENIE_OK;
    default: return GENIE_E_INVALID;
    }
}

int genie_index_set_stage_events(genie_index *ix, void *ev_search_begin, void *ev_search_end)
{
    if (!ix) return GENIE_E_INVALID;
    ix->ev_search_begin = ev_search_begin;
    ix->ev_search_end = ev_search_end;
    return GENIE_OK;
}

const char *genie_strerror(int status)
{
    switch (status) {
    case GENIE_OK: return "ok";
    case GENIE_E_INVALID: return "invalid argument";
    case GENIE_E_ALPHABET: return "base code outside 0..3";
    case GENIE_E_NOMEM: return "out of host memory";
    case GENIE_E_NO_DEVICE: return "index has no device image";
    case GENIE_E_HIP: return "HIP runtime error";
    case GENIE_E_TOO_LONG: return "read or batch larger than the kernels support";
    case GENIE_E_NO_MODEL: return "no RMI model installed";
    case GENIE_E_BAD_BLOB: return "not a serialized GENIE index";
    case GENIE_E_NO_LUT: return "no K-mer table (index built with K = 0, or an image serialized without its seed table)";
    case GENIE_E_CAPACITY: return "output capacity too small";
    case GENIE_W_SEARCH_ONLY: return "GENIE_OPT_SEARCH_ONLY is set: no outputs were produced";
    default: return "unknown status";
    }
}

const char *genie_last_hip_error(void) { return last_hip_error(); }

}  // extern "C"

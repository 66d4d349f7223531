// index_build.hip -- the index image built on the device (genie_index_create_device).
//
// Writes the same bytes as build_host_index + serialize (index_host.cpp, the specification), straight into a caller-owned
// device buffer.  Passes (all on one stream, one synchronisation at the end):
//   1. suffix array by prefix doubling: round 0 ranks the 16-symbol keys (3 bits per symbol, '$' / past the end = 0), each
//      later round the pairs (rank[i], rank[i + h]) -- an LSD radix sort of (key, index) pairs (8-bit digits: per-tile
//      histograms, one scan, a stable scatter that ranks equal digits inside a wave with ballots), a scan of the group heads
//      for the new ranks.  The host cannot see when every rank is distinct without a synchronisation, so it launches the
//      rounds h = 16, 32, ... < n + 1 (enough for any input) and a round after the last needed one finds its row count set
//      to zero and does nothing;
//   2. the LCP of neighbouring suffix-array rows, capped at 16 bases: every per-prefix boundary below (P2-mer entries,
//      the t-mer rows of absent P2-mers, the distinct K-mers) is a row where that LCP drops below the prefix length;
//   3. prefix directory (a binary search per P-mer), its 16-bit-delta test and padtail;
//   4. the header, laid out on the device by the host's own layout_header from the counts found above;
//   5. the sections: packed reference, SaRec rows, dir2 + match table (one thread per P2-mer; overflow block / chain entry
//      numbers from an exclusive scan over the P2-mers in ascending order, as the host hands them out);
//   6. the K-mer hash table.  The host inserts the sorted keys one by one with linear probing; the placement is rebuilt in
//      parallel: a carry scan over the per-slot home counts (carry[j] = max(0, carry[j-1] + homes[j] - 1), cyclic) finds
//      the slots that no probe sequence passes into from the slot before them.  Keys homed between two such slots never
//      leave that stretch and no other key enters it, so each stretch is filled by one thread, inserting its keys in
//      sorted order (a stable radix sort by stretch keeps that order) exactly as the host would.
// Every pass is a function of the codes alone (no atomics decide a value or an order), so the image is deterministic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>

#include "genie_internal.h"

namespace genie {

namespace {

constexpr int kB = 256;                 // threads per block
constexpr int kIpt = 8;                 // elements per thread of a scan / radix tile
constexpr int kTile = kB * kIpt;
constexpr int kLcpCap = 16;             // >= max(P2, K)
constexpr int kSeg = 1024;              // hash-table slots per carry segment

#define HIP_TRY(expr)                                                         \
    do {                                                                      \
        hipError_t e_ = (expr);                                               \
        if (e_ != hipSuccess) { set_hip_error(#expr, (int)e_); return GENIE_E_HIP; } \
    } while (0)

// Device-side counters of one build (front of the scratch).
struct Stats {
    uint32_t sa_count;        // rows while ranks are being refined, 0 once every rank is distinct
    uint32_t bad_code;        // a code > 3 was seen
    uint32_t heads;           // scan total of the last rank pass
    uint32_t lut_keys;        // distinct K-mers
    uint32_t dir16_bad;
    uint32_t need_total;      // compact: P2-mers that want an overflow block; wide: chain entries
    uint32_t lut_slots;
    uint32_t pad;
    uint32_t padtail[8];
};

inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
inline long long al(long long x) { return (x + 255) / 256 * 256; }
inline int bit_length(unsigned long long x) { int b = 0; while (x) { b++; x >>= 1; } return b; }
inline long long tmer_entries(int P2) { return (((long long)1 << (2 * (P2 + 1))) - 4) / 3; }   // 4^1 + ... + 4^P2
__host__ __device__ inline long long tmer_off(int t) { return (((long long)1 << (2 * t)) - 4) / 3; }

// Where each scratch array lives (byte offsets into d_tmp).
struct Scratch {
    long long stats, keys_a, keys_b, vals_a, vals_b, rank, flags, lcp, hist, sums, tfirst, tlast, cut, cut16, need, dir,
        lcode, llo, lhi, hcount, zflag, seg_a, seg_b, seg_cin, total;
    long long rows, nb, sums_n, slots_max, nseg;
};

Scratch scratch_layout(long long n, int K, int P, int P2)
{
    Scratch s;
    s.rows = n + 1;
    s.nb = cdiv(s.rows, kTile);
    const long long nb2 = 1ll << (2 * P2);
    const long long mmax = (K > 0 && n >= K) ? std::min<long long>(n - K + 1, 1ll << (2 * K)) : 0;
    s.slots_max = 2 * mmax + 8;
    s.nseg = cdiv(s.slots_max, kSeg);
    s.sums_n = cdiv(std::max(std::max(s.rows, 256 * s.nb), nb2), kTile) + 1;
    long long o = 0;
    auto take = [&o](long long bytes) { const long long at = o; o = al(o + bytes); return at; };
    s.stats = take(sizeof(Stats));
    s.keys_a = take(8 * s.rows);
    s.keys_b = take(8 * s.rows);
    s.vals_a = take(4 * s.rows);
    s.vals_b = take(4 * s.rows);
    s.rank = take(4 * s.rows);
    s.flags = take(4 * s.rows);
    s.lcp = take(s.rows);
    s.hist = take(4 * 256 * s.nb);
    s.sums = take(4 * s.sums_n);
    s.tfirst = take(4 * tmer_entries(P2));
    s.tlast = take(4 * tmer_entries(P2));
    s.cut = take(nb2);
    s.cut16 = take(nb2);
    s.need = take(4 * nb2);
    s.dir = take(4 * (((long long)1 << (2 * P)) + 1));
    s.lcode = take(4 * std::max(mmax, 1ll));
    s.llo = take(4 * std::max(mmax, 1ll));
    s.lhi = take(4 * std::max(mmax, 1ll));
    s.hcount = take(4 * s.slots_max);
    s.zflag = take(s.slots_max);
    s.seg_a = take(8 * s.nseg);
    s.seg_b = take(8 * s.nseg);
    s.seg_cin = take(8 * s.nseg);
    s.total = o;
    return s;
}

// ------------------------------------------------------------------ device helpers
__device__ __forceinline__ uint32_t base_at(const uint8_t *codes, long long p) { return codes[p] & 3u; }

__device__ __forceinline__ uint64_t code_of(const uint8_t *codes, long long s, int len)
{
    uint64_t c = 0;
    for (int j = 0; j < len; j++) c = (c << 2) | base_at(codes, s + j);
    return c;
}

// 32 bases of the packed reference from position pos (pos >> 5 inside the section; zero past the end)
__device__ __forceinline__ uint64_t window(const RefRec *ref, long long pos)
{
    const RefRec rr = ref[pos >> 5];
    const int sh = (int)(pos & 31) * 2;
    return sh ? (rr.w0 << sh) | (rr.w1 >> (64 - sh)) : rr.w0;
}

__device__ __forceinline__ long long gid() { return (long long)blockIdx.x * blockDim.x + threadIdx.x; }

// exclusive scan of one value per thread over the block; *total = block sum
__device__ uint32_t block_exclusive(uint32_t v, uint32_t *total)
{
    __shared__ uint32_t wsum[kB / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int i = 0; i < kB / 64; i++) {
        if (i < w) before += wsum[i];
        all += wsum[i];
    }
    __syncthreads();
    *total = all;
    return before + x - v;
}

// ------------------------------------------------------------------ exclusive scan of uint32 (count on the device or not)
__device__ __forceinline__ long long count_of(long long nmax, const uint32_t *d_count)
{
    return d_count ? (long long)*d_count : nmax;
}

__global__ void __launch_bounds__(kB) scan_reduce(const uint32_t *__restrict__ in, long long nmax, const uint32_t *d_count,
                                                  uint32_t *__restrict__ sums)
{
    const long long n = count_of(nmax, d_count), base = (long long)blockIdx.x * kTile;
    if (base >= n) return;
    uint32_t acc = 0;
    for (int j = 0; j < kIpt; j++) {
        const long long i = base + (long long)j * kB + threadIdx.x;
        if (i < n) acc += in[i];
    }
    uint32_t tot;
    (void)block_exclusive(acc, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// one block: exclusive scan of the tile sums in place; *d_total = the sum of everything
__global__ void __launch_bounds__(kB) scan_tiles(uint32_t *__restrict__ sums, long long nmax, const uint32_t *d_count,
                                                 uint32_t *d_total)
{
    const long long n = count_of(nmax, d_count), nt = (n + kTile - 1) / kTile;
    const long long per = (nt + kB - 1) / kB, lo = threadIdx.x * per, hi = lo + per < nt ? lo + per : nt;
    uint32_t acc = 0;
    for (long long i = lo; i < hi; i++) acc += sums[i];
    uint32_t tot;
    uint32_t run = block_exclusive(acc, &tot);
    for (long long i = lo; i < hi; i++) {
        const uint32_t v = sums[i];
        sums[i] = run;
        run += v;
    }
    if (threadIdx.x == 0 && d_total) *d_total = tot;
}

// thread t of tile b owns elements b * kTile + t * kIpt .. + kIpt
__global__ void __launch_bounds__(kB) scan_apply(const uint32_t *in, uint32_t *out, long long nmax, const uint32_t *d_count,
                                                 const uint32_t *__restrict__ sums)
{
    const long long n = count_of(nmax, d_count), base = (long long)blockIdx.x * kTile;
    if (base >= n) return;
    const long long first = base + (long long)threadIdx.x * kIpt;
    uint32_t v[kIpt], acc = 0;
    for (int j = 0; j < kIpt; j++) {
        v[j] = first + j < n ? in[first + j] : 0u;
        acc += v[j];
    }
    uint32_t tot;
    uint32_t run = sums[blockIdx.x] + block_exclusive(acc, &tot);
    for (int j = 0; j < kIpt; j++) {
        if (first + j < n) out[first + j] = run;
        run += v[j];
    }
}

// ------------------------------------------------------------------ LSD radix sort of (uint64 key, uint32 value), 8-bit digits
__global__ void __launch_bounds__(kB) radix_hist(const uint64_t *__restrict__ keys, long long nmax, const uint32_t *d_count,
                                                 int shift, uint32_t *__restrict__ hist, long long nb)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long n = count_of(nmax, d_count), base = (long long)blockIdx.x * kTile;
    for (int j = 0; j < kIpt; j++) {
        const long long i = base + (long long)j * kB + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(long long)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];     // digit-major: one scan gives every tile its offsets
}

// Stable scatter: tile elements go in index order, 256 at a time; inside a wave the lanes with the same digit find each
// other with eight ballots, and the waves of the block take their places in wave order.
__global__ void __launch_bounds__(kB) radix_scatter(const uint64_t *__restrict__ kin, const uint32_t *__restrict__ vin,
                                                    uint64_t *__restrict__ kout, uint32_t *__restrict__ vout, long long nmax,
                                                    const uint32_t *d_count, int shift, const uint32_t *__restrict__ hist,
                                                    long long nb)
{
    __shared__ uint32_t next[256];
    __shared__ uint32_t wcnt[kB / 64][256];
    const long long n = count_of(nmax, d_count), base = (long long)blockIdx.x * kTile;
    if (base >= n) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    next[t] = hist[(long long)t * nb + blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1;
    for (int j = 0; j < kIpt; j++) {
        for (int q = 0; q < kB / 64; q++) wcnt[q][t] = 0;
        __syncthreads();
        const long long i = base + (long long)j * kB + t;
        const bool valid = i < n;
        const uint64_t k = valid ? kin[i] : 0;
        const uint32_t v = valid ? vin[i] : 0;
        const uint32_t d = (uint32_t)(k >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const bool set = (d >> b) & 1u;
            const unsigned long long m = __ballot(set);
            peers &= set ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below);
        if (valid && rank == 0) wcnt[w][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        {
            uint32_t run = next[t];
            for (int q = 0; q < kB / 64; q++) {
                const uint32_t c = wcnt[q][t];
                wcnt[q][t] = run;
                run += c;
            }
            next[t] = run;
        }
        __syncthreads();
        if (valid) {
            const uint32_t pos = wcnt[w][d] + rank;
            kout[pos] = k;
            vout[pos] = v;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ suffix array
__global__ void stats_init(Stats *st, long long rows) { st->sa_count = (uint32_t)rows; }

__global__ void __launch_bounds__(kB) check_codes(const uint8_t *__restrict__ codes, long long n, Stats *st)
{
    const long long i = gid();
    if (i < n && codes[i] > 3) atomicOr(&st->bad_code, 1u);
}

__global__ void __launch_bounds__(kB) sa_init(const uint8_t *__restrict__ codes, long long n, uint64_t *__restrict__ keys,
                                              uint32_t *__restrict__ vals)
{
    const long long i = gid();
    if (i > n) return;
    uint64_t k = 0;
    for (int j = 0; j < 16; j++) k = (k << 3) | (i + j < n ? (uint64_t)base_at(codes, i + j) + 1 : 0);
    keys[i] = k;
    vals[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(kB) sa_heads(const uint64_t *__restrict__ keys, const Stats *st, uint32_t *__restrict__ flags)
{
    const long long i = gid();
    if (i >= (long long)st->sa_count) return;
    flags[i] = (i > 0 && keys[i] != keys[i - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(kB) sa_ranks(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                               const uint32_t *__restrict__ excl, const Stats *st, uint32_t *__restrict__ rank)
{
    const long long i = gid();
    if (i >= (long long)st->sa_count) return;
    rank[vals[i]] = excl[i] + ((i > 0 && keys[i] != keys[i - 1]) ? 1u : 0u);
}

__global__ void sa_done(Stats *st, long long rows)
{
    if (st->sa_count && (long long)st->heads == rows - 1) st->sa_count = 0;
}

__global__ void __launch_bounds__(kB) sa_pairs(const uint32_t *__restrict__ vals, const uint32_t *__restrict__ rank,
                                               const Stats *st, long long h, long long rows, int bits, uint64_t *__restrict__ keys)
{
    const long long i = gid();
    if (i >= (long long)st->sa_count) return;
    const long long idx = vals[i], j = idx + h;
    const uint64_t second = j < rows ? (uint64_t)rank[j] + 1 : 0;        // past the end sorts first
    keys[i] = ((uint64_t)rank[idx] << bits) | second;
}

// ------------------------------------------------------------------ per-row products
__global__ void __launch_bounds__(kB) lcp_kernel(const uint8_t *__restrict__ codes, long long n, const int32_t *__restrict__ sa,
                                                 uint8_t *__restrict__ lcp)
{
    const long long r = gid();
    if (r > n) return;
    int L = 0;
    if (r > 0) {
        const long long a = sa[r - 1], b = sa[r];
        while (L < kLcpCap && a + L < n && b + L < n && base_at(codes, a + L) == base_at(codes, b + L)) L++;
    }
    lcp[r] = (uint8_t)L;
}

// rows of every t-mer, t = 1 .. P2: first and last row (rows sharing a prefix are contiguous)
__global__ void __launch_bounds__(kB) tmer_rows(const uint8_t *__restrict__ codes, long long n, const int32_t *__restrict__ sa,
                                                const uint8_t *__restrict__ lcp, int P2, uint32_t *__restrict__ tfirst,
                                                uint32_t *__restrict__ tlast)
{
    const long long r = gid();
    if (r > n) return;
    const long long s = sa[r];
    const int tmax = (int)(n - s < P2 ? n - s : P2);
    if (tmax < 1) return;
    const uint64_t c = code_of(codes, s, tmax);
    const int lp = lcp[r], ln = r < n ? lcp[r + 1] : 0;
    for (int t = lp + 1; t <= tmax; t++) tfirst[tmer_off(t) + (long long)(c >> (2 * (tmax - t)))] = (uint32_t)r;
    for (int t = ln + 1; t <= tmax; t++) tlast[tmer_off(t) + (long long)(c >> (2 * (tmax - t)))] = (uint32_t)r;
}

// dir[x] = rows whose suffix is smaller than the P-mer string x (x = 4^P: all rows)
__global__ void __launch_bounds__(kB) dir_kernel(const uint8_t *__restrict__ codes, long long n, const int32_t *__restrict__ sa,
                                                 int P, uint32_t *__restrict__ dir)
{
    const long long x = gid(), nb = 1ll << (2 * P);
    if (x > nb) return;
    if (x == nb) { dir[x] = (uint32_t)(n + 1); return; }
    long long lo = 0, hi = n + 1;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1, s = sa[mid];
        bool less = false;
        for (int j = 0; j < P; j++) {
            if (s + j >= n) { less = true; break; }
            const uint32_t b = base_at(codes, s + j), d = (uint32_t)(x >> (2 * (P - 1 - j))) & 3u;
            if (b != d) { less = b < d; break; }
        }
        if (less) lo = mid + 1;
        else hi = mid;
    }
    dir[x] = (uint32_t)lo;
}

__global__ void __launch_bounds__(kB) dir16_check(const uint32_t *__restrict__ dir, long long entries, Stats *st)
{
    const long long x = gid();
    if (x < entries && dir[x] - dir[x & ~15ll] > 65535u) atomicOr(&st->dir16_bad, 1u);
}

__global__ void padtail_kernel(const uint8_t *__restrict__ codes, long long n, int P, Stats *st)
{
    for (int l = 0; l < 8; l++)
        st->padtail[l] = (l < P && l <= n) ? (uint32_t)code_of(codes, n - l, l) << (2 * (P - l)) : kNoTail;
}

// P2-mers with a suffix cut short (fewer than P2 + KB, or P2 + 16, bases): only the last 16 suffixes of at least P2 bases
__global__ void cut_kernel(const uint8_t *__restrict__ codes, long long n, int P2, int KB, uint8_t *cut, uint8_t *cut16)
{
    const int j = threadIdx.x;
    const long long s = n - P2 - j;
    if (j >= 16 || s < 0) return;
    const uint64_t c = code_of(codes, s, P2);
    if (P2 + j < P2 + KB) cut[c] = 1;
    cut16[c] = 1;
}

__device__ __forceinline__ uint32_t entry_rows(const uint32_t *tfirst, const uint32_t *tlast, int P2, long long c, uint32_t *first)
{
    const long long at = tmer_off(P2) + c;
    *first = tfirst[at];
    return *first == 0xFFFFFFFFu ? 0u : tlast[at] - *first + 1;
}

// per P2-mer: overflow blocks (compact) / chain entries (wide) it takes, in the host's rules
__global__ void __launch_bounds__(kB) need_kernel(const uint32_t *__restrict__ tfirst, const uint32_t *__restrict__ tlast, int P2,
                                                  bool compact, const uint8_t *__restrict__ cut, uint32_t *__restrict__ need)
{
    const long long c = gid(), nb2 = 1ll << (2 * P2);
    if (c >= nb2) return;
    uint32_t first;
    const uint32_t k = entry_rows(tfirst, tlast, P2, c, &first);
    if (compact) need[c] = (!cut[c] && k > (uint32_t)kM16Keys && k <= (uint32_t)kM16MaxRows) ? 1u : 0u;
    else need[c] = (!cut[c] && k > (uint32_t)kMatchKeys && k <= (uint32_t)kMatchChainRows) ? (k - (kMatchKeys - 1) + 7) / 8 : 0u;
}

// distinct K-mers: a row starts one where the LCP with the row before drops below K
__global__ void __launch_bounds__(kB) kmer_heads(const int32_t *__restrict__ sa, const uint8_t *__restrict__ lcp, long long n,
                                                 int K, uint32_t *__restrict__ flags)
{
    const long long r = gid();
    if (r > n) return;
    flags[r] = (n - sa[r] >= K && lcp[r] < K) ? 1u : 0u;
}

__global__ void __launch_bounds__(kB) kmer_fill(const uint8_t *__restrict__ codes, const int32_t *__restrict__ sa,
                                                const uint8_t *__restrict__ lcp, long long n, int K, const uint32_t *__restrict__ excl,
                                                uint32_t *__restrict__ lcode, int32_t *__restrict__ llo, int32_t *__restrict__ lhi)
{
    const long long r = gid();
    if (r > n) return;
    const long long s = sa[r];
    if (n - s < K) return;
    const bool head = lcp[r] < K, last = r == n || lcp[r + 1] < K;
    if (head) {
        lcode[excl[r]] = (uint32_t)code_of(codes, s, K);
        llo[excl[r]] = (int32_t)r;
    }
    if (last) lhi[excl[r] + (head ? 1 : 0) - 1] = (int32_t)r;
}

// ------------------------------------------------------------------ header (the host's layout, on the device)
__global__ void header_kernel(Stats *st, long long n, int K, int P, int P2, bool compact, int32_t image_flags, BlobHeader *hdr)
{
    ImageShape s;
    s.n = n;
    s.K = K;
    s.P = P;
    s.P2 = P2;
    s.flags = (st->dir16_bad ? 0 : kFlagDir16) | (compact ? kFlagCompactTable : 0);
    s.sa_rows = n + 1;
    s.ref_recs = (n + 31) / 32 + 3;
    s.dir_entries = (1ll << (2 * P)) + 1;
    s.dir2_entries = 1ll << (2 * P2);
    s.lut_keys = st->lut_keys;
    s.lut_slots = (K > 0 && n >= K) ? 2 * (int64_t)st->lut_keys + 8 : 8;
    st->lut_slots = (uint32_t)s.lut_slots;
    s.rmi_models = 0;
    s.rmi_err_entries = 0;
    s.nlev = 0;
    for (int l = 0; l < GENIE_MAX_RMI_LEVELS; l++) s.rmi_size[l] = s.rmi_scale[l] = 0;
    for (int l = 0; l <= GENIE_MAX_RMI_LEVELS; l++) s.rmi_off[l] = 0;
    for (int l = 0; l < 8; l++) s.padtail[l] = st->padtail[l];
    s.mtab_entries = s.dir2_entries + (compact ? 0 : (int64_t)st->need_total);
    s.ov_entries = compact ? 1 + (st->need_total < kM16MaxOv - 1 ? (int64_t)st->need_total : kM16MaxOv - 1) : 0;
    layout_header(s, hdr, image_flags);
}

// ------------------------------------------------------------------ sections
__global__ void __launch_bounds__(kB) ref_kernel(const uint8_t *__restrict__ codes, long long n, uint8_t *image)
{
    const BlobHeader *hdr = reinterpret_cast<const BlobHeader *>(image);
    const long long i = gid();
    if (i >= hdr->ref_recs) return;
    uint64_t w[2] = {0, 0};
    for (int h = 0; h < 2; h++) {
        const long long p0 = (i + h) * 32;
        for (int j = 0; j < 32 && p0 + j < n; j++) w[h] |= (uint64_t)base_at(codes, p0 + j) << (62 - 2 * j);
    }
    reinterpret_cast<RefRec *>(image + hdr->off_ref)[i] = RefRec{w[0], w[1]};
}

__device__ __forceinline__ uint64_t sarec_key(const RefRec *ref, long long n, int P, long long s)
{
    return s + P < n ? window(ref, s + P) : 0;
}

__global__ void __launch_bounds__(kB) sarec_kernel(const int32_t *__restrict__ sa, long long n, int P, uint8_t *image)
{
    const BlobHeader *hdr = reinterpret_cast<const BlobHeader *>(image);
    const long long r = gid();
    if (r > n) return;
    const RefRec *ref = reinterpret_cast<const RefRec *>(image + hdr->off_ref);
    const int32_t s = sa[r];
    reinterpret_cast<SaRec *>(image + hdr->off_sa)[r] = SaRec{s, 0, sarec_key(ref, n, P, s)};
}

__global__ void __launch_bounds__(kB) dir_copy(const uint32_t *__restrict__ dir, uint8_t *image)
{
    const BlobHeader *hdr = reinterpret_cast<const BlobHeader *>(image);
    const long long x = gid();
    if (x < hdr->dir_entries) reinterpret_cast<uint32_t *>(image + hdr->off_dir)[x] = dir[x];
}

// one thread per P2-mer: its HeadRec and match-table entry (+ overflow block / chain entries), as build_host_index
__global__ void __launch_bounds__(kB) p2_entries(const int32_t *__restrict__ sa, long long n, int P, int P2, bool compact,
                                                 const uint32_t *__restrict__ tfirst, const uint32_t *__restrict__ tlast,
                                                 const uint8_t *__restrict__ cut, const uint8_t *__restrict__ cut16,
                                                 const uint32_t *__restrict__ excl, uint8_t *image)
{
    const BlobHeader *hdr = reinterpret_cast<const BlobHeader *>(image);
    const long long c = gid(), nb2 = 1ll << (2 * P2);
    if (c >= nb2) return;
    const RefRec *ref = reinterpret_cast<const RefRec *>(image + hdr->off_ref);
    uint32_t first;
    const uint32_t k = entry_rows(tfirst, tlast, P2, c, &first);
    HeadRec hr{0, 0, 0};
    if (k) {
        const long long s = sa[first];
        hr = HeadRec{first, k | ((n - s < P + 32) ? kHeadShort : 0u), sarec_key(ref, n, P, s)};
    }
    reinterpret_cast<HeadRec *>(image + hdr->off_dir2)[c] = hr;
    // absent: the longest prefix that does occur, and its rows
    int t = 0;
    uint32_t plb = 0, plast = 0;
    if (!k) {
        for (t = P2 - 1; t >= 1; t--) {
            const long long at = tmer_off(t) + (c >> (2 * (P2 - t)));
            if (tfirst[at] != 0xFFFFFFFFu) {
                plb = tfirst[at];
                plast = tlast[at];
                break;
            }
        }
    }
    // the 16 bases after the first P2 of row first + i (zero past the end)
    auto key32 = [&](uint32_t i) { return (uint32_t)(window(ref, (long long)sa[first + i] + P2) >> 32); };
    if (compact) {
        MatchRec16 m{0, {0, 0, 0, 0, 0, 0}};
        if (!k) {
            m.w0 = plb | ((uint32_t)t << 28);
            m.key[0] = (uint16_t)(plast & 0xFFFFu);
            m.key[1] = (uint16_t)(plast >> 16);
        } else if (k <= 3u && !cut16[c]) {                       // wide keys: three 32-bit keys in dwords 1..3
            uint32_t k32[3];
            k32[0] = k32[1] = k32[2] = key32(0);
            for (uint32_t i = 1; i < k; i++) k32[i] = key32(i);
            for (int i = 0; i < 3; i++) {
                m.key[2 * i] = (uint16_t)(k32[i] & 0xFFFFu);
                m.key[2 * i + 1] = (uint16_t)(k32[i] >> 16);
            }
            m.w0 = first | (k << 24) | (kM16Wide << 28);
        } else {
            uint32_t ovf = 0;
            if (!cut[c] && k > (uint32_t)kM16Keys && k <= (uint32_t)kM16MaxRows) {
                const uint32_t e = 1 + excl[c];
                ovf = e < (uint32_t)kM16MaxOv ? e : 0;
            }
            const uint16_t key0 = (uint16_t)(key32(0) >> 16);
            for (int j = 0; j < kM16Keys; j++) m.key[j] = key0;
            if (ovf) {
                for (uint32_t i = 1; i < (uint32_t)kM16Keys - 1; i++) m.key[i] = (uint16_t)(key32(i) >> 16);
                MatchOv16 o;
                const uint16_t key5 = (uint16_t)(key32(kM16Keys - 1) >> 16);
                for (int j = 0; j < kM16OvKeys; j++) o.key[j] = key5;
                for (uint32_t i = kM16Keys; i < k; i++) o.key[i - (kM16Keys - 1)] = (uint16_t)(key32(i) >> 16);
                reinterpret_cast<MatchOv16 *>(image + hdr->off_ov)[ovf] = o;
                m.key[kM16Keys - 1] = (uint16_t)ovf;
                m.w0 = first | (kM16More << 24) | ((k - 7u) << 28);
            } else {
                const uint32_t nk = k < (uint32_t)kM16Keys ? k : (uint32_t)kM16Keys;
                for (uint32_t i = 1; i < nk; i++) m.key[i] = (uint16_t)(key32(i) >> 16);
                if (k <= (uint32_t)kM16Keys) m.w0 = first | (k << 24) | ((cut[c] ? kM16General : 0u) << 28);
                else m.w0 = first | ((uint32_t)kM16Keys << 24) | (kM16General << 28);   // the rows decide
            }
        }
        reinterpret_cast<MatchRec16 *>(image + hdr->off_mtab)[c] = m;
        return;
    }
    MatchRec *mtab = reinterpret_cast<MatchRec *>(image + hdr->off_mtab);
    MatchRec m{0, 0, {0, 0, 0, 0, 0, 0}};
    if (!k) {
        m.meta = (uint32_t)t;
        m.lb = plb;
        m.key[0] = plast;
    } else {
        m.lb = first;
        const bool chain = !cut[c] && k > (uint32_t)kMatchKeys && k <= (uint32_t)kMatchChainRows;
        const uint32_t key0 = key32(0);
        for (int j = 0; j < kMatchKeys; j++) m.key[j] = key0;
        if (!chain) {
            const uint32_t nk = k < (uint32_t)kMatchKeys ? k : (uint32_t)kMatchKeys;
            for (uint32_t i = 1; i < nk; i++) m.key[i] = key32(i);
        } else {
            for (uint32_t i = 1; i < (uint32_t)kMatchKeys - 1; i++) m.key[i] = key32(i);
            const uint32_t idx = (uint32_t)nb2 + excl[c], extra = (k - (kMatchKeys - 1) + 7) / 8;
            m.key[kMatchKeys - 1] = idx;
            for (uint32_t e = 0; e < extra; e++) {
                uint32_t fw[8];
                for (int j = 0; j < 8; j++) {
                    const uint32_t row = (kMatchKeys - 1) + e * 8 + j;
                    fw[j] = row < k ? key32(row) : key0;
                }
                MatchRec fill;
                __builtin_memcpy(&fill, fw, sizeof(fill));
                mtab[idx + e] = fill;
            }
        }
        const uint32_t slow = (k > (uint32_t)kMatchKeys || cut[c]) ? kMatchSlow | (chain ? kMatchMore : 0u) : 0u;
        m.meta = slow | (uint32_t)P2 | (slow ? 0u : 0x1Fu << 8) | ((k < 255 ? k : 255u) << 24);
    }
    mtab[c] = m;
}

// ------------------------------------------------------------------ K-mer hash table
__global__ void __launch_bounds__(kB) lut_clear(uint8_t *image)
{
    const BlobHeader *hdr = reinterpret_cast<const BlobHeader *>(image);
    const long long i = gid();
    if (i < hdr->lut_slots) reinterpret_cast<LutSlot *>(image + hdr->off_lut)[i] = LutSlot{0, -1, -1, 0};
}

__global__ void __launch_bounds__(kB) lut_homes(const uint32_t *__restrict__ lcode, const Stats *st, uint32_t *__restrict__ hcount)
{
    const long long i = gid();
    if (i < (long long)st->lut_keys) atomicAdd(&hcount[lut_hash(lcode[i], st->lut_slots)], 1u);
}

// carry(x) over a run of slots = max(a, x + b); one slot with h homes: max(0, x + h - 1)
struct Carry {
    long long a, b;
};
__device__ __forceinline__ Carry then(Carry f, Carry g) { return Carry{g.a > f.a + g.b ? g.a : f.a + g.b, f.b + g.b}; }
__device__ __forceinline__ long long apply(Carry f, long long x) { return f.a > x + f.b ? f.a : x + f.b; }

__global__ void __launch_bounds__(kB) carry_segments(const uint32_t *__restrict__ hcount, const Stats *st, long long *seg_a,
                                                     long long *seg_b)
{
    const long long g = gid(), S = st->lut_slots;
    if (g * kSeg >= S) return;
    Carry f{0, 0};
    for (long long j = g * kSeg; j < S && j < (g + 1) * kSeg; j++) f = then(f, Carry{0, (long long)hcount[j] - 1});
    seg_a[g] = f.a;
    seg_b[g] = f.b;
}

// one block: carry into every segment; the carry into slot 0 is the carry out of the last slot (an empty slot exists, so
// one pass from zero finds it exactly)
__global__ void __launch_bounds__(kB) carry_scan(const long long *seg_a, const long long *seg_b, const Stats *st, long long *seg_cin)
{
    __shared__ long long sa_[kB], sb_[kB];
    const long long nseg = (st->lut_slots + kSeg - 1) / kSeg;
    const long long per = (nseg + kB - 1) / kB, lo = threadIdx.x * per, hi = lo + per < nseg ? lo + per : nseg;
    Carry f{0, 0};
    for (long long i = lo; i < hi; i++) f = then(f, Carry{seg_a[i], seg_b[i]});
    sa_[threadIdx.x] = f.a;
    sb_[threadIdx.x] = f.b;
    __syncthreads();
    for (int o = 1; o < kB; o <<= 1) {                      // inclusive scan under composition
        Carry mine{sa_[threadIdx.x], sb_[threadIdx.x]};
        if ((int)threadIdx.x >= o) mine = then(Carry{sa_[threadIdx.x - o], sb_[threadIdx.x - o]}, mine);
        __syncthreads();
        sa_[threadIdx.x] = mine.a;
        sb_[threadIdx.x] = mine.b;
        __syncthreads();
    }
    const long long c_end = apply(Carry{sa_[kB - 1], sb_[kB - 1]}, 0);
    long long x = threadIdx.x ? apply(Carry{sa_[threadIdx.x - 1], sb_[threadIdx.x - 1]}, c_end) : c_end;
    for (long long i = lo; i < hi; i++) {
        seg_cin[i] = x;
        x = apply(Carry{seg_a[i], seg_b[i]}, x);
    }
}

__global__ void __launch_bounds__(kB) carry_slots(const uint32_t *__restrict__ hcount, const long long *seg_cin, const Stats *st,
                                                  uint8_t *__restrict__ zflag)
{
    const long long g = gid(), S = st->lut_slots;
    if (g * kSeg >= S) return;
    long long x = seg_cin[g];
    for (long long j = g * kSeg; j < S && j < (g + 1) * kSeg; j++) {
        zflag[j] = x == 0 ? 1 : 0;
        x = x + (long long)hcount[j] - 1;
        if (x < 0) x = 0;
    }
}

// the stretch of a key: the nearest slot at or before its home (cyclic) with no carry into it
__global__ void __launch_bounds__(kB) lut_groups(const uint32_t *__restrict__ lcode, const uint8_t *__restrict__ zflag, const Stats *st,
                                                 uint64_t *__restrict__ gkey, uint32_t *__restrict__ gval)
{
    const long long i = gid();
    if (i >= (long long)st->lut_keys) return;
    const uint32_t S = st->lut_slots;
    uint32_t g = lut_hash(lcode[i], S);
    while (!zflag[g]) g = g ? g - 1 : S - 1;
    gkey[i] = g;
    gval[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(kB) lut_place(const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gval,
                                                const uint32_t *__restrict__ lcode, const int32_t *__restrict__ llo,
                                                const int32_t *__restrict__ lhi, const Stats *st, uint8_t *image)
{
    const BlobHeader *hdr = reinterpret_cast<const BlobHeader *>(image);
    const long long p = gid(), m = st->lut_keys;
    if (p >= m || (p > 0 && gkey[p - 1] == gkey[p])) return;
    LutSlot *lut = reinterpret_cast<LutSlot *>(image + hdr->off_lut);
    const uint32_t S = st->lut_slots;
    for (long long q = p; q < m && gkey[q] == gkey[p]; q++) {
        const uint32_t i = gval[q];
        uint32_t slot = lut_hash(lcode[i], S);
        while (lut[slot].lo >= 0) slot = slot + 1 == S ? 0 : slot + 1;
        lut[slot] = LutSlot{lcode[i], llo[i], lhi[i], 0};
    }
}

unsigned grid_of(long long n) { return (unsigned)std::max<long long>(1, cdiv(n, kB)); }

struct Launcher {
    hipStream_t s;
    const Scratch &L;
    uint8_t *tmp;
    template <class T> T *at(long long off) const { return reinterpret_cast<T *>(tmp + off); }

    // exclusive scan of in[0 .. count) into out (may alias); count = *d_count when given, else nmax
    void scan(const uint32_t *in, uint32_t *out, long long nmax, const uint32_t *d_count, uint32_t *d_total) const
    {
        const long long tiles = std::max(1ll, cdiv(nmax, kTile));
        uint32_t *sums = at<uint32_t>(L.sums);
        hipLaunchKernelGGL(scan_reduce, dim3((unsigned)tiles), dim3(kB), 0, s, in, nmax, d_count, sums);
        hipLaunchKernelGGL(scan_tiles, dim3(1), dim3(kB), 0, s, sums, nmax, d_count, d_total);
        hipLaunchKernelGGL(scan_apply, dim3((unsigned)tiles), dim3(kB), 0, s, in, out, nmax, d_count, (const uint32_t *)sums);
    }

    // stable sort of (ka, va)[0 .. count) by the low `bits` key bits; the result is back in ka / va (even pass count)
    void sort(uint64_t *ka, uint32_t *va, uint64_t *kb, uint32_t *vb, long long nmax, const uint32_t *d_count, int bits) const
    {
        int passes = (bits + 7) / 8;
        passes += passes & 1;
        const long long nb = std::max(1ll, cdiv(nmax, kTile));
        uint32_t *hist = at<uint32_t>(L.hist);
        for (int p = 0; p < passes; p++) {
            hipLaunchKernelGGL(radix_hist, dim3((unsigned)nb), dim3(kB), 0, s, (const uint64_t *)ka, nmax, d_count, 8 * p, hist, nb);
            scan(hist, hist, 256 * nb, nullptr, nullptr);
            hipLaunchKernelGGL(radix_scatter, dim3((unsigned)nb), dim3(kB), 0, s, (const uint64_t *)ka, (const uint32_t *)va, kb, vb,
                               nmax, d_count, 8 * p, (const uint32_t *)hist, nb);
            std::swap(ka, kb);
            std::swap(va, vb);
        }
    }
};

}  // namespace

int64_t device_image_bound(int64_t n, int32_t K, int32_t P, int32_t P2, bool compact)
{
    const long long rows = n + 1, mmax = (K > 0 && n >= K) ? std::min<long long>(n - K + 1, 1ll << (2 * K)) : 0;
    ImageShape s{};
    s.n = n;
    s.K = K;
    s.P = P;
    s.P2 = P2;
    s.flags = compact ? kFlagCompactTable : 0;
    s.sa_rows = rows;
    s.ref_recs = (n + 31) / 32 + 3;
    s.dir_entries = (1ll << (2 * P)) + 1;
    s.dir2_entries = 1ll << (2 * P2);
    s.lut_keys = mmax;
    s.lut_slots = 2 * mmax + 8;
    // an overflow block / chain entry serves at least 7 rows
    s.mtab_entries = s.dir2_entries + (compact ? 0 : rows / 7 + 1);
    s.ov_entries = compact ? std::min<long long>(kM16MaxOv, 1 + rows / 7 + 1) : 0;
    BlobHeader hdr;
    layout_header(s, &hdr, 0);
    return hdr.total_bytes;
}

int64_t device_build_tmp_bytes(int64_t n, int32_t K, int32_t P, int32_t P2) { return scratch_layout(n, K, P, P2).total; }

int device_build(const uint8_t *d_codes, int64_t n, int32_t K, int32_t P, int32_t P2, bool compact, int32_t image_flags,
                 void *d_image, int64_t image_cap, void *d_tmp, int64_t tmp_bytes, void *stream, BlobHeader *hdr_out)
{
    const Scratch L = scratch_layout(n, K, P, P2);
    if (tmp_bytes < L.total) return GENIE_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    Launcher go{s, L, (uint8_t *)d_tmp};
    uint8_t *image = (uint8_t *)d_image;
    const long long rows = L.rows, nb2 = 1ll << (2 * P2), ndir = (1ll << (2 * P)) + 1;
    const int KB = compact ? 8 : 16;
    const bool lut = K > 0 && n >= K;
    Stats *st = go.at<Stats>(L.stats);
    uint64_t *ka = go.at<uint64_t>(L.keys_a), *kb = go.at<uint64_t>(L.keys_b);
    uint32_t *va = go.at<uint32_t>(L.vals_a), *vb = go.at<uint32_t>(L.vals_b), *rank = go.at<uint32_t>(L.rank);
    uint32_t *flags = go.at<uint32_t>(L.flags);
    const int32_t *sa = go.at<int32_t>(L.vals_a);
    uint8_t *lcp = go.at<uint8_t>(L.lcp);
    uint32_t *tfirst = go.at<uint32_t>(L.tfirst), *tlast = go.at<uint32_t>(L.tlast), *need = go.at<uint32_t>(L.need);
    uint8_t *cut = go.at<uint8_t>(L.cut), *cut16 = go.at<uint8_t>(L.cut16);
    uint32_t *dir = go.at<uint32_t>(L.dir);

    HIP_TRY(hipMemsetAsync(d_image, 0, (size_t)std::min<int64_t>(image_cap, device_image_bound(n, K, P, P2, compact)), s));
    HIP_TRY(hipMemsetAsync(st, 0, sizeof(Stats), s));
    hipLaunchKernelGGL(stats_init, dim3(1), dim3(1), 0, s, st, rows);
    hipLaunchKernelGGL(check_codes, dim3(grid_of(n)), dim3(kB), 0, s, d_codes, (long long)n, st);

    // 1. suffix array: 16-symbol keys, then (rank[i], rank[i + h]) pairs until every rank is distinct
    const int rbits = bit_length((unsigned long long)rows);            // rank + 1 <= rows < 2^rbits
    hipLaunchKernelGGL(sa_init, dim3(grid_of(rows)), dim3(kB), 0, s, d_codes, (long long)n, ka, va);
    for (long long h = 0;; h = h ? 2 * h : 16) {
        if (h) {
            if (h >= rows) break;
            hipLaunchKernelGGL(sa_pairs, dim3(grid_of(rows)), dim3(kB), 0, s, (const uint32_t *)va, (const uint32_t *)rank,
                               (const Stats *)st, h, rows, rbits, ka);
        }
        go.sort(ka, va, kb, vb, rows, &st->sa_count, h ? 2 * rbits : 48);
        hipLaunchKernelGGL(sa_heads, dim3(grid_of(rows)), dim3(kB), 0, s, (const uint64_t *)ka, (const Stats *)st, flags);
        go.scan(flags, flags, rows, &st->sa_count, &st->heads);
        hipLaunchKernelGGL(sa_ranks, dim3(grid_of(rows)), dim3(kB), 0, s, (const uint64_t *)ka, (const uint32_t *)va,
                           (const uint32_t *)flags, (const Stats *)st, rank);
        hipLaunchKernelGGL(sa_done, dim3(1), dim3(1), 0, s, st, rows);
    }
    HIP_TRY(hipGetLastError());

    // 2. neighbour LCPs, t-mer rows; 3. prefix directory
    hipLaunchKernelGGL(lcp_kernel, dim3(grid_of(rows)), dim3(kB), 0, s, d_codes, (long long)n, sa, lcp);
    HIP_TRY(hipMemsetAsync(tfirst, 0xFF, 4 * (size_t)tmer_entries(P2), s));
    hipLaunchKernelGGL(tmer_rows, dim3(grid_of(rows)), dim3(kB), 0, s, d_codes, (long long)n, sa, (const uint8_t *)lcp, P2, tfirst, tlast);
    hipLaunchKernelGGL(dir_kernel, dim3(grid_of(ndir)), dim3(kB), 0, s, d_codes, (long long)n, sa, P, dir);
    hipLaunchKernelGGL(dir16_check, dim3(grid_of(ndir)), dim3(kB), 0, s, (const uint32_t *)dir, ndir, st);
    hipLaunchKernelGGL(padtail_kernel, dim3(1), dim3(1), 0, s, d_codes, (long long)n, P, st);
    HIP_TRY(hipMemsetAsync(cut, 0, (size_t)nb2, s));
    HIP_TRY(hipMemsetAsync(cut16, 0, (size_t)nb2, s));
    hipLaunchKernelGGL(cut_kernel, dim3(1), dim3(64), 0, s, d_codes, (long long)n, P2, KB, cut, cut16);
    hipLaunchKernelGGL(need_kernel, dim3(grid_of(nb2)), dim3(kB), 0, s, (const uint32_t *)tfirst, (const uint32_t *)tlast, P2, compact,
                       (const uint8_t *)cut, need);
    go.scan(need, need, nb2, nullptr, &st->need_total);
    uint32_t *lcode = go.at<uint32_t>(L.lcode);
    int32_t *llo = go.at<int32_t>(L.llo), *lhi = go.at<int32_t>(L.lhi);
    if (lut) {
        hipLaunchKernelGGL(kmer_heads, dim3(grid_of(rows)), dim3(kB), 0, s, sa, (const uint8_t *)lcp, (long long)n, K, flags);
        go.scan(flags, flags, rows, nullptr, &st->lut_keys);
        hipLaunchKernelGGL(kmer_fill, dim3(grid_of(rows)), dim3(kB), 0, s, d_codes, sa, (const uint8_t *)lcp, (long long)n, K,
                           (const uint32_t *)flags, lcode, llo, lhi);
    }
    HIP_TRY(hipGetLastError());

    // 4. header; 5. sections
    hipLaunchKernelGGL(header_kernel, dim3(1), dim3(1), 0, s, st, (long long)n, K, P, P2, compact, image_flags,
                       reinterpret_cast<BlobHeader *>(image));
    const long long ref_recs = (n + 31) / 32 + 3;
    hipLaunchKernelGGL(ref_kernel, dim3(grid_of(ref_recs)), dim3(kB), 0, s, d_codes, (long long)n, image);
    hipLaunchKernelGGL(sarec_kernel, dim3(grid_of(rows)), dim3(kB), 0, s, sa, (long long)n, P, image);
    hipLaunchKernelGGL(dir_copy, dim3(grid_of(ndir)), dim3(kB), 0, s, (const uint32_t *)dir, image);
    hipLaunchKernelGGL(p2_entries, dim3(grid_of(nb2)), dim3(kB), 0, s, sa, (long long)n, P, P2, compact, (const uint32_t *)tfirst,
                       (const uint32_t *)tlast, (const uint8_t *)cut, (const uint8_t *)cut16, (const uint32_t *)need, image);
    hipLaunchKernelGGL(lut_clear, dim3(grid_of(lut && !(image_flags & GENIE_IMAGE_NO_SEED_TABLE) ? L.slots_max : 8)), dim3(kB), 0, s, image);
    HIP_TRY(hipGetLastError());

    // 6. K-mer hash table: the host's sequential linear-probing placement, stretch by stretch
    if (lut && !(image_flags & GENIE_IMAGE_NO_SEED_TABLE)) {
        uint32_t *hcount = go.at<uint32_t>(L.hcount);
        uint8_t *zflag = go.at<uint8_t>(L.zflag);
        long long *seg_a = go.at<long long>(L.seg_a), *seg_b = go.at<long long>(L.seg_b), *seg_cin = go.at<long long>(L.seg_cin);
        HIP_TRY(hipMemsetAsync(hcount, 0, 4 * (size_t)L.slots_max, s));
        const long long mmax = (L.slots_max - 8) / 2;
        hipLaunchKernelGGL(lut_homes, dim3(grid_of(mmax)), dim3(kB), 0, s, (const uint32_t *)lcode, (const Stats *)st, hcount);
        hipLaunchKernelGGL(carry_segments, dim3(grid_of(L.nseg)), dim3(kB), 0, s, (const uint32_t *)hcount, (const Stats *)st, seg_a, seg_b);
        hipLaunchKernelGGL(carry_scan, dim3(1), dim3(kB), 0, s, (const long long *)seg_a, (const long long *)seg_b, (const Stats *)st, seg_cin);
        hipLaunchKernelGGL(carry_slots, dim3(grid_of(L.nseg)), dim3(kB), 0, s, (const uint32_t *)hcount, (const long long *)seg_cin,
                           (const Stats *)st, zflag);
        // group keys / values reuse the suffix-array sort buffers (va still holds the suffix array)
        uint64_t *gka = ka, *gkb = kb;
        uint32_t *gva = rank, *gvb = vb;
        hipLaunchKernelGGL(lut_groups, dim3(grid_of(mmax)), dim3(kB), 0, s, (const uint32_t *)lcode, (const uint8_t *)zflag,
                           (const Stats *)st, gka, gva);
        go.sort(gka, gva, gkb, gvb, mmax, &st->lut_keys, bit_length((unsigned long long)L.slots_max));
        hipLaunchKernelGGL(lut_place, dim3(grid_of(mmax)), dim3(kB), 0, s, (const uint64_t *)gka, (const uint32_t *)gva,
                           (const uint32_t *)lcode, (const int32_t *)llo, (const int32_t *)lhi, (const Stats *)st, image);
        HIP_TRY(hipGetLastError());
    }

    Stats hst;
    HIP_TRY(hipMemcpyAsync(hdr_out, image, sizeof(BlobHeader), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&hst, st, sizeof(Stats), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hst.bad_code) return GENIE_E_ALPHABET;
    if (hdr_out->total_bytes > image_cap) return GENIE_E_CAPACITY;
    return GENIE_OK;
}

}  // namespace genie

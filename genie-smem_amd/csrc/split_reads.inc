// split_reads.inc -- genie_find_smems_split: the SMEMs of reads that contain breaks (included by kernels.hip, inside
// namespace genie; uses its launch plumbing).
//
// A break is a position whose code is > 3 or whose base never occurs in the reference; a segment is a maximal run of
// positions that are not breaks.  No exact match covers a break, so the SMEMs of a read are the SMEMs of its segments,
// segment after segment.  None of the tuned kernels changes: the segments are gathered into a batch of their own and the
// batch goes through launch_find_smems_csr in BWA mode.
//   K_S0 split_check_kernel    one pass over the read bytes, 16 per lane: is there a break, an empty read or a length out
//                              of range anywhere?  The host reads the answer (the one synchronisation of the fast path).
//                              Nothing: the reads themselves are the batch, launch_find_smems_csr as genie_find_smems_csr.
//   K_S1 split_count_kernel    one wave per read, ballots over 64 bases at a time: segments per read, their sums per
//                              group of kSplitGroup reads, and three batch totals (segments, longest segment, lengths out
//                              of range), which the host reads.
//   scan_block_sums_kernel     over the group sums; K_S2 split_offsets_kernel: first segment of every read.
//   per pass of at most C segments (C from the workspace and the longest segment):
//   K_S3 split_fill_kernel     one wave per read that has segments in the pass: segment table (read, start, length) and
//                              the segment's bases, gathered into rows of the longest segment's length;
//   launch_find_smems_csr      on the gathered batch, rows written straight behind the previous pass's;
//   K_S4 split_remap_kernel    start / end += the segment's start (one thread per segment); per-read offsets = the
//                              offset of the read's first segment (one thread per read).  A read's segments are
//                              consecutive in the batch, so this is one gather, no sort.
//   Between passes the host reads the pass's row total (one synchronisation per extra pass).
namespace {

constexpr int kSplitWaves = 8;          // waves per block of the segmentation kernels (one read each)
constexpr int kSplitGroup = kSplitWaves;  // reads per group sum of the segment scan

// totals of K_S1, int64 words at the front of the workspace
enum { kSplitSegs = 0, kSplitLongest = 1, kSplitBadLen = 2 };   // word 4: the flags of K_S0 (32-bit)

// Bit b set: base b occurs in the reference.  The prefix directory counts, below entry x, the suffixes of P or more bases
// whose P-mer is < x and the tail suffixes (fewer than P bases) whose A-padded code is <= x.  So the block
// [dir[b << 2(P-1)], dir[(b+1) << 2(P-1)]) holds the suffixes of P or more bases that start with b plus the tail suffixes
// whose padded code lies in (b << 2(P-1), (b+1) << 2(P-1)]; those are subtracted (padtail[l] = padded code of the tail of
// l bases).  A base that occurs only in the last P-1 positions is found in the tail itself.
__device__ __forceinline__ uint32_t split_present_bases(const DevIndex &ix)
{
    const int sh = 2 * (ix.P - 1);
    const int L = ix.n < ix.P - 1 ? ix.n : ix.P - 1;
    uint32_t m = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const uint32_t x0 = (uint32_t)b << sh, x1 = (uint32_t)(b + 1) << sh;
        uint32_t tails = 0;
        for (int l = 0; l <= L; l++) tails += (ix.padtail[l] > x0 && ix.padtail[l] <= x1) ? 1u : 0u;
        if (ix.dir[x1] - ix.dir[x0] > tails) m |= 1u << b;
    }
    const uint32_t t = ix.padtail[L] >> (2 * (ix.P - L));
    for (int j = 0; j < L; j++) m |= 1u << ((t >> (2 * j)) & 3u);
    return m;
}

// Bit b set: base b occurs at least k times in the reference (min_occ.inc: a base that is not "rare at k").  The counts are
// those split_present_bases tests against zero -- the suffixes of P or more bases from the directory, the last P-1 positions
// from the tail -- so k == 1 gives its mask.
__device__ __forceinline__ uint32_t split_usable_bases(const DevIndex &ix, int k)
{
    const int sh = 2 * (ix.P - 1);
    const int L = ix.n < ix.P - 1 ? ix.n : ix.P - 1;
    const uint32_t t = ix.padtail[L] >> (2 * (ix.P - L));
    uint32_t m = 0;
    for (int b = 0; b < 4; b++) {
        const uint32_t x0 = (uint32_t)b << sh, x1 = (uint32_t)(b + 1) << sh;
        long long cnt = (long long)ix.dir[x1] - (long long)ix.dir[x0];
        for (int l = 0; l <= L; l++) cnt -= (ix.padtail[l] > x0 && ix.padtail[l] <= x1) ? 1 : 0;
        for (int j = 0; j < L; j++) cnt += ((t >> (2 * j)) & 3u) == (uint32_t)b ? 1 : 0;
        if (cnt >= k) m |= 1u << b;
    }
    return m;
}

// Walk one read with the calling wave, 64 bases per ballot (four loads in flight per lane).  For every position that is
// not a break the lane holding it calls base(i, k, start) (k = its segment's index in the read, start = the segment's
// first position); for every segment the lane holding its last base (lane 0 for one that ends at a 64-base boundary)
// calls end(k, start, len).  Returns the read's segment count (wave-uniform).
template <class FBase, class FEnd>
__device__ __forceinline__ int split_walk(const uint8_t *__restrict__ read, int len, uint32_t present, FBase &&base, FEnd &&end)
{
    const int lane = threadIdx.x & (kWave - 1);
    int nstart = 0;           // segments started before the current chunk
    int run_start = 0;        // first position of the segment open at the chunk boundary
    bool open = false;
    for (int b0 = 0; b0 < len; b0 += 4 * kWave) {
        uint32_t c[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = b0 + q * kWave + lane;
            c[q] = i < len ? read[i] : 255u;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int cb = b0 + q * kWave;
            if (cb >= len) break;
            const bool ok = c[q] < 4u && ((present >> c[q]) & 1u);
            const uint64_t good = __ballot(ok);
            const uint64_t starts = good & ~((good << 1) | (open ? 1ull : 0ull));
            if (open && !(good & 1ull) && lane == 0) end(nstart - 1, run_start, cb - run_start);
            const uint64_t le = lane == 63 ? ~0ull : (2ull << lane) - 1;
            const uint64_t sl = starts & le;
            const int k = sl ? nstart + __popcll(sl) - 1 : nstart - 1;
            const int st = sl ? cb + 63 - __clzll(sl) : run_start;
            if (ok) {
                base(cb + lane, k, st);
                if (lane < 63 && !((good >> (lane + 1)) & 1ull)) end(k, st, cb + lane - st + 1);
            }
            nstart += __popcll(starts);
            open = (good >> 63) & 1ull;
            if (open && starts) run_start = cb + 63 - __clzll(starts);
        }
    }
    if (open && lane == 0) end(nstart - 1, run_start, len - run_start);
    return nstart;
}

__device__ __forceinline__ int split_len(const int32_t *lens, long long r, int fixed_len)
{
    const int l = lens ? lens[r] : fixed_len;
    return (l < 0 || l > fixed_len) ? -1 : l;
}

// K_S0: does any read need the general path?  One pass over the read bytes at full width (16 bytes per lane; the bytes
// before the first and after the last 16-byte boundary one at a time): flags[0] != 0 if a position inside a read is a break,
// a read is empty, or a length lies outside [0, fixed_len] (then flags[1] != 0 too).  Persistent blocks; one atomic per
// block that found something.
__device__ __forceinline__ bool split_byte_ok(uint32_t c, uint32_t present) { return c < 4u && ((present >> c) & 1u); }

__global__ void __launch_bounds__(256) split_check_kernel(DevIndex ix, const uint8_t *__restrict__ reads,
                                                          const int32_t *__restrict__ lens, long long N, int stride,
                                                          int fixed_len, unsigned int *__restrict__ flags)
{
    __shared__ unsigned int found;
    if (threadIdx.x == 0) found = 0;
    __syncthreads();
    const uint32_t present = split_present_bases(ix);
    unsigned int f = 0;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (long long)gridDim.x * blockDim.x;
    if (lens) {
        for (long long r = tid; r < N; r += nthreads) {
            const int l = lens[r];
            f |= (l < 0 || l > fixed_len) ? 3u : (l == 0 ? 1u : 0u);
        }
    }
    const long long total = N * (long long)stride;
    const uintptr_t base = reinterpret_cast<uintptr_t>(reads);
    const long long head = (long long)(((base + 15) & ~(uintptr_t)15) - base);
    const long long words = total > head ? (total - head) / 16 : 0;
    const long long tail0 = head + words * 16;
    // a byte at position pos of its read (len bases); advances to the next byte of the batch
    auto check_byte = [&](uint32_t c, long long &r, int &pos, int &len) {
        if (pos < len && !split_byte_ok(c, present)) f |= 1u;
        if (++pos == stride) {
            pos = 0;
            ++r;
            if (r < N) len = lens ? lens[r] : fixed_len;
        }
    };
    if (!lens && stride == fixed_len && present == 0xFu) {
        // dense reads, every base in the reference: a break is a byte with a bit above bit 1
        for (long long w = tid; w < words; w += nthreads) {
            const uint4 v = *reinterpret_cast<const uint4 *>(reads + head + w * 16);
            f |= ((v.x | v.y | v.z | v.w) & 0xFCFCFCFCu) ? 1u : 0u;
        }
    } else {
        for (long long w = tid; w < words; w += nthreads) {
            const long long o = head + w * 16;
            const uint4 v = *reinterpret_cast<const uint4 *>(reads + o);
            long long r = o / stride;
            int pos = (int)(o - r * stride);
            int len = lens ? lens[r] : fixed_len;
            const uint32_t dw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; k++) check_byte((dw[k >> 2] >> (8 * (k & 3))) & 0xFFu, r, pos, len);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 32) {                // the unaligned head and tail
        const long long o = threadIdx.x < 16 ? (long long)threadIdx.x : tail0 + (threadIdx.x - 16);
        const bool mine = threadIdx.x < 16 ? o < head && o < total : o < total;
        if (mine) {
            long long r = o / stride;
            int pos = (int)(o - r * stride);
            int len = lens ? lens[r] : fixed_len;
            check_byte(reads[o], r, pos, len);
        }
    }
    if (f) atomicOr(&found, f);
    __syncthreads();
    if (threadIdx.x == 0 && found) atomicOr(flags, found);
}

// K_S1: persistent blocks; group g = reads [g * kSplitGroup, +kSplitGroup), one wave per read.
__global__ void __launch_bounds__(kSplitWaves * 64) split_count_kernel(DevIndex ix, const uint8_t *__restrict__ reads,
                                                                       const int32_t *__restrict__ lens, long long N, int stride,
                                                                       int fixed_len, int32_t *__restrict__ nseg,
                                                                       unsigned long long *__restrict__ gsum,
                                                                       unsigned long long *__restrict__ totals)
{
    __shared__ int part[kSplitWaves][3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    const uint32_t present = split_present_bases(ix);
    const long long groups = (N + kSplitGroup - 1) / kSplitGroup;
    long long segs = 0;
    int longest = 0, bad = 0;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long r = g * kSplitGroup + wave;
        int cnt = 0;
        if (r < N) {
            int len = split_len(lens, r, fixed_len);
            if (len < 0) { bad++; len = 0; }
            int lng = 0;
            cnt = split_walk(reads + r * (long long)stride, len, present, [](int, int, int) {},
                             [&](int, int, int l) { lng = l > lng ? l : lng; });
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                lng = max(lng, __shfl_xor(lng, off, kWave));
            }
            longest = max(longest, lng);
            if (lane == 0) nseg[r] = cnt;
        }
        if (lane == 0) part[wave][0] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long s = 0;
            for (int w = 0; w < kSplitWaves; w++) s += (unsigned)part[w][0];
            gsum[g] = s;
            segs += (long long)s;
        }
        __syncthreads();
    }
    if (lane == 0) { part[wave][1] = longest; part[wave][2] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int lg = 0, bd = 0;
        for (int w = 0; w < kSplitWaves; w++) { lg = max(lg, part[w][1]); bd += part[w][2]; }
        if (segs) atomicAdd(totals + kSplitSegs, (unsigned long long)segs);
        if (lg) atomicMax(totals + kSplitLongest, (unsigned long long)lg);
        if (bd) atomicAdd(totals + kSplitBadLen, (unsigned long long)bd);
    }
}

// K_S2: segoff[r] = index of read r's first segment in the whole batch (segoff[N] = all segments)
__global__ void __launch_bounds__(256) split_offsets_kernel(const int32_t *__restrict__ nseg, const unsigned long long *__restrict__ gsum,
                                                            long long N, long long *__restrict__ segoff)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const long long g0 = r / kSplitGroup * kSplitGroup;
    long long o = (long long)gsum[r / kSplitGroup];
    for (long long q = g0; q < r; q++) o += nseg[q];
    segoff[r] = o;
    if (r == N - 1) segoff[N] = o + nseg[r];
}

struct SplitPass {
    long long p0, p1;           // segments [p0, p1) of the whole batch
    int32_t *seg_read, *seg_start, *seg_len;
    uint8_t *gbuf;              // (p1 - p0) rows of gstride bytes
    int gstride;
};

// K_S3: one wave per read; reads without a segment in the pass leave at once
__global__ void __launch_bounds__(kSplitWaves * 64) split_fill_kernel(DevIndex ix, const uint8_t *__restrict__ reads,
                                                                      const int32_t *__restrict__ lens, long long N, int stride,
                                                                      int fixed_len, const long long *__restrict__ segoff,
                                                                      SplitPass ps)
{
    const long long r = (long long)blockIdx.x * kSplitWaves + (threadIdx.x >> 6);
    if (r >= N) return;
    const long long f = segoff[r], l = segoff[r + 1];
    if (l <= ps.p0 || f >= ps.p1) return;
    const int len = split_len(lens, r, fixed_len);
    if (len <= 0) return;
    const uint8_t *read = reads + r * (long long)stride;
    const uint32_t present = split_present_bases(ix);
    split_walk(read, len, present,
               [&](int i, int k, int st) {
                   const long long s = f + k;
                   if (s >= ps.p0 && s < ps.p1) ps.gbuf[(s - ps.p0) * ps.gstride + (i - st)] = read[i];
               },
               [&](int k, int st, int sl) {
                   const long long s = f + k;
                   if (s >= ps.p0 && s < ps.p1) {
                       ps.seg_read[s - ps.p0] = (int32_t)r;
                       ps.seg_start[s - ps.p0] = st;
                       ps.seg_len[s - ps.p0] = sl;
                   }
               });
}

// K_S4: rows of the pass (they start at d_rows + row0; the caller's capacity counts from d_rows) get their segment's
// start; reads whose first segment is in the pass (or, in the last pass, that have none left) get their offset.
__global__ void __launch_bounds__(256) split_remap_kernel(SplitPass ps, const long long *__restrict__ local_off,
                                                          const int32_t *__restrict__ seg_status, long long row0,
                                                          int4 *__restrict__ rows, long long out_cap_rows,
                                                          const long long *__restrict__ segoff, long long N, bool last,
                                                          long long *__restrict__ offsets, int32_t *__restrict__ status)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long C = ps.p1 - ps.p0;
    if (i < C) {
        const int st = ps.seg_start[i];
        const long long a = row0 + local_off[i], b = row0 + local_off[i + 1];
        for (long long t = a; t < b && t < out_cap_rows; t++) {
            int4 v = rows[t];
            v.x += st;
            v.y += st;
            rows[t] = v;
        }
        if (status && seg_status[i] != GENIE_READ_OK) status[ps.seg_read[i]] = seg_status[i];
    }
    if (i < N) {
        const long long f = segoff[i];
        if (f >= ps.p0 && (f < ps.p1 || (last && f == ps.p1))) offsets[i] = row0 + local_off[f - ps.p0];
        if (last && i == N - 1) offsets[N] = row0 + local_off[C];
    }
}

// Workspace of the split call: the totals and segment scan for N reads, then one pass area (below).
struct SplitFixedArea {
    unsigned long long *totals;      // K_S1's totals and K_S0's flags
    int32_t *nseg;
    unsigned long long *gsum;
    long long *segoff;
};

inline int64_t split_fixed_layout(uint8_t *base, int64_t N, SplitFixedArea *a)
{
    Carver c{base};
    c.take(a->totals, 256);
    c.take(a->nseg, N * 4);
    c.take(a->gsum, ((N + kSplitGroup - 1) / kSplitGroup + 1) * 8);
    c.take(a->segoff, (N + 1) * 8);
    return c.at;
}

inline int split_gstride(int max_len) { return std::max(16, (max_len + 15) & ~15); }

// a pass of C segments of at most max_len bases: segment table, segment status, the pass's CSR offsets, the gathered
// bases and the find_smems workspace of the batch
struct SplitPassArea {
    int32_t *seg_read, *seg_start, *seg_len, *seg_status;
    long long *local_off;
    uint8_t *gbuf;
    uint8_t *csr_ws;
    int64_t csr_ws_bytes;
};

inline int64_t split_pass_layout(uint8_t *base, int64_t C, int max_len, SplitPassArea *a)
{
    Carver c{base};
    c.take(a->seg_read, C * 4);
    c.take(a->seg_start, C * 4);
    c.take(a->seg_len, C * 4);
    c.take(a->seg_status, C * 4);
    c.take(a->local_off, (C + 1) * 8);
    c.take(a->gbuf, C * (int64_t)split_gstride(max_len) + 256);
    a->csr_ws_bytes = find_smems_workspace_bytes(C, max_len);
    c.take(a->csr_ws, a->csr_ws_bytes);
    return c.at;
}

}  // namespace

int64_t find_smems_split_workspace_bytes(int64_t N, int32_t max_len)
{
    SplitFixedArea f;
    SplitPassArea a;
    return split_fixed_layout(nullptr, N, &f) + split_pass_layout(nullptr, std::max<int64_t>(N, 1), max_len, &a);
}

int launch_find_smems_split(const genie_index *ix, const uint8_t *d_reads, const int32_t *d_lens, int64_t N, int32_t stride,
                            int32_t fixed_len, int32_t min_len, int64_t *d_offsets, int32_t *d_rows, int64_t out_cap_rows,
                            int32_t *d_status, void *d_ws, int64_t ws_bytes, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, 8, s));
        return GENIE_OK;
    }
    SplitFixedArea f;
    const int64_t fixed = split_fixed_layout(static_cast<uint8_t *>(d_ws), N, &f);
    uint8_t *p = static_cast<uint8_t *>(d_ws) + fixed;        // the pass area
    const int64_t pass_avail = ws_bytes - fixed;
    const long long groups = (N + kSplitGroup - 1) / kSplitGroup;

    const int cus = ix->num_cus > 0 ? ix->num_cus : 256;
    HIP_TRY(hipMemsetAsync(f.totals, 0, 40, s));
    if (fixed_len > 0) {                                       // fast path: no break and no empty read -> the reads are the batch
        unsigned int *flags = reinterpret_cast<unsigned int *>(f.totals + 4);
        const long long work = std::max<long long>(N, N * (long long)stride / 16);
        LAUNCH(split_check_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>((work + 255) / 256, (long long)cus * 8))),
               dim3(256), 0, s, ix->dev, d_reads, d_lens, (long long)N, stride, fixed_len, flags);
        unsigned int fl = 0;
        HIP_TRY(hipMemcpyAsync(&fl, flags, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (fl & 2u) return GENIE_E_INVALID;                   // a length outside [0, fixed_len]
        if (fl == 0)
            return launch_find_smems_csr(ix, GENIE_MODE_BWA, {d_reads, d_lens, N, stride, fixed_len, min_len, d_status, p, pass_avail},
                                         d_offsets, d_rows, out_cap_rows, stream);
    }
    LAUNCH(split_count_kernel, dim3((unsigned)std::min<long long>(groups, (long long)cus * 8)), dim3(kSplitWaves * 64), 0, s,
           ix->dev, d_reads, d_lens, (long long)N, stride, fixed_len, f.nseg, f.gsum, f.totals);
    unsigned long long tot[3];
    HIP_TRY(hipMemcpyAsync(tot, f.totals, sizeof(tot), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (tot[kSplitBadLen]) return GENIE_E_INVALID;             // a length outside [0, fixed_len]

    if (d_status) HIP_TRY(hipMemsetAsync(d_status, 0, N * 4, s));
    const long long S = (long long)tot[kSplitSegs];
    if (S == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, (N + 1) * 8, s));
        return GENIE_OK;
    }
    const int M = (int)tot[kSplitLongest];
    // segments per pass: as many as the workspace holds at this longest segment (at least N: the caller sized it for N reads
    // of fixed_len >= M bases)
    SplitPassArea a;
    const long long C = pass_size(std::max<long long>(N, 1), S, [&](long long c) { return split_pass_layout(nullptr, c, M, &a) <= pass_avail; });
    LAUNCH(scan_block_sums_kernel, dim3(1), dim3(kScanBlock), 0, s, f.gsum, groups);
    LAUNCH(split_offsets_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, f.nseg, f.gsum, (long long)N, f.segoff);

    split_pass_layout(p, C, M, &a);
    long long row0 = 0;
    for (long long p0 = 0; p0 < S; p0 += C) {
        const long long p1 = std::min(S, p0 + C);
        const bool last = p1 == S;
        SplitPass ps{p0, p1, a.seg_read, a.seg_start, a.seg_len, a.gbuf, split_gstride(M)};
        LAUNCH(split_fill_kernel, dim3((unsigned)((N + kSplitWaves - 1) / kSplitWaves)), dim3(kSplitWaves * 64), 0, s,
               ix->dev, d_reads, d_lens, (long long)N, stride, fixed_len, f.segoff, ps);
        const long long cap_left = std::max(0ll, (long long)out_cap_rows - row0);
        int rc = launch_find_smems_csr(ix, GENIE_MODE_BWA, {a.gbuf, a.seg_len, p1 - p0, ps.gstride, M, min_len, a.seg_status, a.csr_ws,
                                                            a.csr_ws_bytes},
                                       reinterpret_cast<int64_t *>(a.local_off), cap_left > 0 ? d_rows + 4 * row0 : d_rows, cap_left, stream);
        if (rc) return rc;
        const long long threads = std::max(p1 - p0, (long long)N);
        LAUNCH(split_remap_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, ps,
               static_cast<const long long *>(a.local_off), static_cast<const int32_t *>(a.seg_status), row0,
               reinterpret_cast<int4 *>(d_rows), (long long)out_cap_rows, static_cast<const long long *>(f.segoff),
               (long long)N, last, reinterpret_cast<long long *>(d_offsets), d_status);
        if (!last) {
            long long pass_rows = 0;
            HIP_TRY(hipMemcpyAsync(&pass_rows, a.local_off + (p1 - p0), 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            row0 += pass_rows;
        }
    }
    return GENIE_OK;
}

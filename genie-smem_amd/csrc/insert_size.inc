// insert_size.inc -- genie_insert_size_stats: the insert-size distribution of a paired batch, estimated from the pairs whose two
// heads map confidently to one contig (included by align.inc behind pairs.inc, inside namespace genie).  The definition is the
// header's; DESIGN.md section 29 has the reasoning.  The heads, their combination type and their span are pairs.inc's own
// (pair_mate, pair_values, pair_combo), so the two calls cannot disagree about what a pair is.
//   IS0 chain_check_kernel    the record offsets; the host reads the flag: the call's one synchronisation
//   IS1 isize_sample_kernel   one lane per pair, grid-stride: (t, s) of the pair into d_samples and into a histogram.  A block
//                             counts the spans below kIsizeLds in LDS and adds its non-zero bins to the global histogram when it
//                             is done; spans from kIsizeLds on go to the global histogram at once.  The four totals are summed
//                             over the block, then added once.
//   IS2 isize_finish_kernel   one block, kIsizeGroup lanes per type: each lane sums a contiguous run of bins, a scan of those sums
//                             places the three ranks, two more passes over [lo_b, hi_b] give n_in, S and SS, one lane bisects std
//                             and writes the type's row
// Every sum here is an integer add, so the histogram, the totals and all that follows are the same in whatever order the blocks
// arrive.  Nothing is sorted.
namespace {

#ifdef GENIE_ISIZE_NO_LDS
constexpr int kIsizeLds = 0;                                  // a build for measuring what the LDS histogram saves
#else
constexpr int kIsizeLds = GENIE_ISIZE_LDS_BINS;               // spans below this are counted in LDS
#endif
constexpr int kIsizeBlock = 512;                              // IS1: three blocks of 48 KB on a CU, six waves per SIMD
constexpr int kIsizeGroup = 256;                              // IS2: lanes per type
constexpr int kIsizeGroupWaves = kIsizeGroup / kWave;
static_assert(3 * (3 * kIsizeLds * 4 + 4 * (kIsizeBlock / kWave) * 8) <= 160 * 1024, "three blocks per CU");
static_assert(GENIE_ISIZE_LDS_BINS > 0 && GENIE_ISIZE_LDS_BINS <= GENIE_WINDOW_MAX / 2, "the LDS range lies inside the largest max_span");

struct IsizeArea {
    int *flag;                            // IS0's verdict
    unsigned long long *totals;           // 4
    unsigned int *hist;                   // 3 (max_span + 1): a pair is counted once and there are fewer than 2^30 pairs
};

inline int64_t isize_layout(uint8_t *base, int64_t max_span, IsizeArea *a)
{
    Carver c{base};
    c.take(a->flag, 8);
    c.take(a->totals, 32);
    c.take(a->hist, 3 * (max_span + 1) * 4);
    return c.at;
}

__global__ void __launch_bounds__(kIsizeBlock) isize_sample_kernel(PairInput in, int min_mapq, int max_span, int2 *__restrict__ samples,
                                                                   unsigned int *__restrict__ hist, unsigned long long *__restrict__ totals)
{
    __shared__ unsigned int bins[kIsizeLds > 0 ? 3 * kIsizeLds : 1];
    __shared__ unsigned long long wsum[4][kIsizeBlock / kWave];
    const int held = kIsizeLds < max_span + 1 ? kIsizeLds : max_span + 1;          // bins of a type that LDS holds
    for (int i = threadIdx.x; i < 3 * held; i += kIsizeBlock) bins[i] = 0;
    __syncthreads();
    const PairParams any{7, 0, 0, 0, 0, 0, 0, 0};                                   // the type and the span need no parameter
    unsigned long long both = 0, taken = 0, low = 0, off = 0;
    for (long long k = (long long)blockIdx.x * kIsizeBlock + threadIdx.x; k < in.P; k += (long long)gridDim.x * kIsizeBlock) {
        const PairMate m0 = pair_mate(in, 2 * k), m1 = pair_mate(in, 2 * k + 1);
        int t = -1, s = 0;
        if (m0.n > 0 && m1.n > 0) {
            both++;
            const int4 h0 = pair_values(in, m0.lo, in.rec[3 * (long long)m0.lo].w), h1 = pair_values(in, m1.lo, in.rec[3 * (long long)m1.lo].w);
            const int q0 = (int)sel_clamp(in.rec[3 * (long long)m0.lo + 2].w, 0, 60), q1 = (int)sel_clamp(in.rec[3 * (long long)m1.lo + 2].w, 0, 60);
            const PairCombo c = pair_combo(h0, h1, any);
            if (c.type < 0 || c.type > 2 || c.span < 1 || c.span > max_span) {
                off++;
            } else if (q0 < min_mapq || q1 < min_mapq) {
                low++;
            } else {
                taken++;
                t = c.type;
                s = (int)c.span;
                if (s < held)
                    atomicAdd(&bins[t * held + s], 1u);
                else
                    atomicAdd(&hist[(long long)t * (max_span + 1) + s], 1u);
            }
        }
        if (samples) samples[k] = make_int2(t, s);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * held; i += kIsizeBlock) {
        const unsigned int c = bins[i];
        if (c) atomicAdd(&hist[(long long)(i / held) * (max_span + 1) + i % held], c);
    }
    both = wave_sum64(both);
    taken = wave_sum64(taken);
    low = wave_sum64(low);
    off = wave_sum64(off);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        wsum[0][threadIdx.x / kWave] = both;
        wsum[1][threadIdx.x / kWave] = taken;
        wsum[2][threadIdx.x / kWave] = low;
        wsum[3][threadIdx.x / kWave] = off;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long all = 0;
        for (int w = 0; w < kIsizeBlock / kWave; w++) all += wsum[threadIdx.x][w];
        if (all) atomicAdd(&totals[threadIdx.x], all);
    }
}

// the sum of v over the kIsizeGroup lanes of type t, in every one of them; all three groups call it together
__device__ __forceinline__ unsigned long long isize_group_sum(unsigned long long v, unsigned long long (*part)[kIsizeGroupWaves], int t, int w,
                                                              int lane)
{
    v = wave_sum64(v);
    __syncthreads();                                                 // the sums before have been read
    if (lane == 0) part[t][w] = v;
    __syncthreads();
    unsigned long long all = 0;
    for (int i = 0; i < kIsizeGroupWaves; i++) all += part[t][i];
    return all;
}

__global__ void __launch_bounds__(3 * kIsizeGroup) isize_finish_kernel(const unsigned int *__restrict__ hist,
                                                                       const unsigned long long *__restrict__ sums, int max_span,
                                                                       int min_samples, long long *__restrict__ stats,
                                                                       long long *__restrict__ totals)
{
    __shared__ unsigned long long part[3][kIsizeGroupWaves];
    __shared__ long long quart[3][3];
    const int t = threadIdx.x / kIsizeGroup, g = threadIdx.x % kIsizeGroup, lane = g & (kWave - 1), w = g / kWave;
    const int nbins = max_span + 1, per = (nbins + kIsizeGroup - 1) / kIsizeGroup;
    const unsigned int *h = hist + (long long)t * nbins;
    const int lo = g * per < nbins ? g * per : nbins, hi = lo + per < nbins ? lo + per : nbins;
    if (threadIdx.x < 9) (&quart[0][0])[threadIdx.x] = 0;
    // the lane's run of bins, and the samples below it
    unsigned long long mine = 0;
    for (int s = lo; s < hi; s++) mine += h[s];
    const unsigned long long incl = wave_inclusive_scan64(mine, lane);
    if (lane == kWave - 1) part[t][w] = incl;
    __syncthreads();
    unsigned long long below = incl - mine, n = 0, n_most = 0;
    for (int i = 0; i < kIsizeGroupWaves; i++) {
        if (i < w) below += part[t][i];
        n += part[t][i];
    }
    for (int u = 0; u < 3; u++) {
        unsigned long long nu = 0;
        for (int i = 0; i < kIsizeGroupWaves; i++) nu += part[u][i];
        n_most = nu > n_most ? nu : n_most;
    }
    // the three ranks: each falls into the run of exactly one lane
    if (n > 0 && mine > 0) {
        const unsigned long long r1 = (n + 1) / 4 < n - 1 ? (n + 1) / 4 : n - 1, r2 = n / 2, r3 = (3 * n + 1) / 4 < n - 1 ? (3 * n + 1) / 4 : n - 1;
        unsigned long long cum = below;
        for (int s = lo; s < hi; s++) {
            const unsigned long long c = h[s];
            if (cum <= r1 && r1 < cum + c) quart[t][0] = s;
            if (cum <= r2 && r2 < cum + c) quart[t][1] = s;
            if (cum <= r3 && r3 < cum + c) quart[t][2] = s;
            cum += c;
        }
    }
    __syncthreads();
    const long long q25 = quart[t][0], q50 = quart[t][1], q75 = quart[t][2], iqr = q75 - q25;
    const long long lo_b = q25 - GENIE_ISIZE_OUTLIER_IQR * iqr > 1 ? q25 - GENIE_ISIZE_OUTLIER_IQR * iqr : 1, hi_b = q75 + GENIE_ISIZE_OUTLIER_IQR * iqr;
    const long long last = n > 0 ? (hi_b < max_span ? hi_b : max_span) : 0;        // no sample: nothing to pass over
    unsigned long long n_in = 0, S = 0;
    for (long long s = lo_b + g; s <= last; s += kIsizeGroup) {
        const unsigned long long c = h[s];
        n_in += c;
        S += c * (unsigned long long)s;
    }
    n_in = isize_group_sum(n_in, part, t, w, lane);
    S = isize_group_sum(S, part, t, w, lane);
    const long long mean = n_in > 0 ? (long long)((2 * S + n_in) / (2 * n_in)) : 0;
    unsigned long long SS = 0;
    for (long long s = lo_b + g; s <= last; s += kIsizeGroup) {
        const long long d = s - mean;
        SS += (unsigned long long)h[s] * (unsigned long long)(d * d);
    }
    SS = isize_group_sum(SS, part, t, w, lane);
    if (g == 0) {
        long long a = 0, b = max_span;                               // the smallest d with d d n_in >= SS: max_span is one
        while (a < b) {
            const long long mid = (a + b) >> 1;
            if ((unsigned long long)(mid * mid) * n_in >= SS) b = mid; else a = mid + 1;
        }
        const long long std_ = a;
        const bool ok = n >= (unsigned long long)min_samples && 20 * n >= n_most;
        long long w_lo = q25 - GENIE_ISIZE_WINDOW_IQR * iqr, w_hi = q75 + GENIE_ISIZE_WINDOW_IQR * iqr;
        w_lo = w_lo < mean - GENIE_ISIZE_WINDOW_STD * std_ ? w_lo : mean - GENIE_ISIZE_WINDOW_STD * std_;
        w_hi = w_hi > mean + GENIE_ISIZE_WINDOW_STD * std_ ? w_hi : mean + GENIE_ISIZE_WINDOW_STD * std_;
        w_lo = w_lo > 0 ? w_lo : 0;
        w_hi = w_hi < max_span ? w_hi : max_span;
        long long *row = stats + 12 * t;
        row[0] = (long long)n;
        row[1] = ok ? 1 : 0;
        row[2] = q25;
        row[3] = q50;
        row[4] = q75;
        row[5] = ok ? lo_b : 0;
        row[6] = ok ? hi_b : 0;
        row[7] = ok ? (long long)n_in : 0;
        row[8] = ok ? mean : 0;
        row[9] = ok ? std_ : 0;
        row[10] = ok ? w_lo : 0;
        row[11] = ok ? w_hi : 0;
    }
    if (totals && threadIdx.x < 4) totals[threadIdx.x] = (long long)sums[threadIdx.x];
}

}  // namespace

int64_t insert_size_stats_workspace_bytes(int64_t N, int32_t max_span)
{
    (void)N;                                                         // nothing is kept per pair
    IsizeArea a;
    return isize_layout(nullptr, max_span, &a);
}

int launch_insert_size_stats(const genie_index *ix, const IsizeBatch &b, const IsizeOut &out, void *ws, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = b.N, P = N / 2;
    if (N == 0) {
        HIP_TRY(hipMemsetAsync(out.stats, 0, 3 * 12 * 8, s));
        if (out.totals) HIP_TRY(hipMemsetAsync(out.totals, 0, 32, s));
        return GENIE_OK;
    }
    IsizeArea a;
    const int64_t used = isize_layout(static_cast<uint8_t *>(ws), b.max_span, &a);
    const long long *so = reinterpret_cast<const long long *>(b.sel_offsets);
    HIP_TRY(hipMemsetAsync(ws, 0, used, s));                         // the verdict, the totals and the histogram
    LAUNCH_BLOCKS(chain_check_kernel, (N + 1 + 255) / 256, 256, 0, s, so, (long long)N, 0x7fffffffffffffffll, a.flag);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, a.flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return GENIE_E_INVALID;
    const PairInput in{so, (long long)N, (long long)P, reinterpret_cast<const int4 *>(b.records), (long long)b.n_records, nullptr, 0};
    const long long want = (P + kIsizeBlock - 1) / kIsizeBlock, most = (long long)(ix->num_cus > 0 ? ix->num_cus : 256) * 3;
    LAUNCH(isize_sample_kernel, dim3((unsigned)std::min(want, most)), dim3(kIsizeBlock), 0, s, in, (int)b.min_mapq, (int)b.max_span,
           reinterpret_cast<int2 *>(out.samples), a.hist, a.totals);
    LAUNCH(isize_finish_kernel, dim3(1), dim3(3 * kIsizeGroup), 0, s, static_cast<const unsigned int *>(a.hist),
           static_cast<const unsigned long long *>(a.totals), (int)b.max_span, (int)b.min_samples,
           reinterpret_cast<long long *>(out.stats), reinterpret_cast<long long *>(out.totals));
    return GENIE_OK;
}

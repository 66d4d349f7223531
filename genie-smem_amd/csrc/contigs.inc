// contigs.inc -- a reference of several sequences: the contig table, its lookup, genie_contigs_validate,
// genie_contig_coords and genie_locate_contigs (included by kernels.hip in front of mems.inc, inside namespace genie).
//
// The table is the caller's: n_contigs + 1 int64 offsets into the concatenation, the convention of the read CSR (contig c
// is T[off[c] .. off[c+1]), empty contigs allowed).  The contig of a position t < n is the LAST c with off[c] <= t.
//
// The lookup.  Every kernel that needs it stages samples of the table in LDS as int32, clamped to [0, n]: sample i is
// off[i << shift], shift the smallest at which the samples fit.  A lane bisects the samples, then, only when shift > 0, the
// 2^shift table entries between two samples in global memory (shift loads, L2 resident: the table of 10^4 contigs is 80 KB).
// The kernels of 256 threads (coords, locate) stage up to kCtgSamples values: a table of up to 1023 contigs is answered from
// LDS alone.  The MEM walks (1024 threads) choose per block between that staging and one of up to kCtgWalkSamples values, by
// the seed rows of the block's positions (mem_walk_kernel; measured in DESIGN.md section 18).
// Memory safety on ANY table contents: the bisections move indices inside [0, n_contigs] whatever the values say, the
// contig is clamped to n_contigs - 1 before off[c + 1] is read, every value is clamped to [0, n] and room to >= 0; a table
// that genie_contigs_validate refuses gives undefined answers and no access outside the table, the index or the outputs.
namespace {

constexpr int kCtgSamples = 1024;         // staged values per block of 256 threads (coords, locate): 4 KB of LDS
constexpr int kCtgWalkSamples = 12288;    // ... of the MEM walks: 48 KB; their 1024 threads leave room for two blocks per CU anyway

struct CtgTab {
    const long long *off;                 // n_contigs + 1
    int nc, shift, ns;                    // contigs; sample i = off[i << shift]; samples = (nc >> shift) + 1, as many as the kernel stages
};

inline CtgTab ctg_tab(const int64_t *d_off, int64_t n_contigs, int samples = kCtgSamples)
{
    CtgTab g{reinterpret_cast<const long long *>(d_off), (int)n_contigs, 0, 0};
    while ((g.nc >> g.shift) + 1 > samples) g.shift++;
    g.ns = (g.nc >> g.shift) + 1;
    return g;
}

// The MEM walks choose per block between two stagings of the same table (mem_walk_kernel)
struct CtgPair {
    CtgTab big, small;
};

inline size_t ctg_lds_bytes(const CtgTab &g) { return sizeof(int) * (size_t)g.ns; }

struct CtgHit {
    int c, start, room;                   // the contig of t, its first position, the bases from t to its end (>= 0)
};

__device__ __forceinline__ int ctg_clamp(long long x, int n) { return x < 0 ? 0 : (x > n ? n : (int)x); }

// Every thread of the block calls it; the samples are readable behind it.
__device__ __forceinline__ void ctg_stage(const CtgTab &g, int n, int *__restrict__ cs)
{
    for (int i = threadIdx.x; i < g.ns; i += blockDim.x) cs[i] = ctg_clamp(g.off[(long long)i << g.shift], n);
    __syncthreads();
}

__device__ __forceinline__ CtgHit ctg_find(const CtgTab &g, const int *__restrict__ cs, int n, int t)
{
    int lo = 0, hi = g.ns;                                       // cs[lo] <= t (off[0] = 0); cs[hi] > t or hi == ns
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cs[mid] <= t) lo = mid; else hi = mid;
    }
    int c, a, b;
    if (g.shift == 0) {                                          // the whole table is staged: ns == nc + 1
        c = lo < g.nc - 1 ? lo : g.nc - 1;
        a = cs[c];
        b = cs[c + 1];
    } else {
        int glo = lo << g.shift, ghi = g.nc - glo > (1 << g.shift) ? glo + (1 << g.shift) : g.nc;
        while (ghi - glo > 1) {
            const int mid = glo + ((ghi - glo) >> 1);
            if (ctg_clamp(g.off[mid], n) <= t) glo = mid; else ghi = mid;
        }
        c = glo < g.nc - 1 ? glo : g.nc - 1;
        a = ctg_clamp(g.off[c], n);
        b = ctg_clamp(g.off[c + 1], n);
    }
    const int room = b - t;
    return CtgHit{c, a, room > 0 ? room : 0};
}

// genie_contigs_validate: off[0] == 0 (1), non-decreasing (2), off[n_contigs] == n (4)
__global__ void __launch_bounds__(256) ctg_validate_kernel(const long long *__restrict__ off, long long nc, long long n,
                                                           unsigned int *__restrict__ bad)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned int err = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i <= nc; i += stride) {
        const long long x = off[i];
        if (i == 0 && x != 0) err |= 1u;
        if (i == nc && x != n) err |= 4u;
        if (i < nc && x > off[i + 1]) err |= 2u;
    }
    if (err) atomicOr(bad, err);
}

// genie_contig_coords: one lane per element
__global__ void __launch_bounds__(256) ctg_coords_kernel(DevIndex ix, CtgTab g, const int32_t *__restrict__ pos, int stride,
                                                         long long count, int32_t *__restrict__ out)
{
    extern __shared__ int ctg_lds[];
    ctg_stage(g, ix.n, ctg_lds);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int p = pos[i * stride];
    int c = -1, o = -1;
    if (p >= 1 && p <= ix.n) {
        const CtgHit h = ctg_find(g, ctg_lds, ix.n, p - 1);
        c = h.c;
        o = p - h.start;
    }
    out[2 * i] = c;
    out[2 * i + 1] = o;
}

// What a lane needs of its SMEM row to walk the interval
struct LcRow {
    int lo, cnt, len;
};

__device__ __forceinline__ LcRow lc_row(const DevIndex &ix, const int4 *__restrict__ rows, long long g, long long S)
{
    LcRow q{0, 0, 0};
    if (g < S) {
        const int4 r = rows[g];
        const int hi = r.w < ix.n ? r.w : ix.n;                  // a row number beyond the suffix array is not followed
        q.lo = r.z;
        q.cnt = (r.z >= 0 && hi >= r.z) ? hi - r.z + 1 : 0;
        q.len = r.y - r.x;
    }
    return q;
}

// Is the occurrence at suffix-array row r inside one contig?  2: it bridges two (or runs off the last); 0: the $ suffix.
__device__ __forceinline__ int lc_hit(const DevIndex &ix, const CtgTab &g, const int *__restrict__ cs, int r, int len, int2 &out)
{
    const int t = ix.sa[r].s;
    if (t >= ix.n) return 0;
    const CtgHit h = ctg_find(g, cs, ix.n, t);
    out = make_int2(h.c, t - h.start + 1);
    return len <= h.room ? 1 : 2;
}

// genie_locate_contigs, count (FILL false) and fill: one lane per interval up to 32 rows, the whole wave beyond
// (locate_scatter_kernel's shape).  The same predicate, lc_hit, decides both.
template <bool FILL>
__global__ void __launch_bounds__(256) lc_walk_kernel(DevIndex ix, CtgTab g, const int4 *__restrict__ rows, long long S,
                                                      int32_t *__restrict__ counts, unsigned long long *__restrict__ dropped,
                                                      const long long *__restrict__ offsets, int2 *__restrict__ hits, long long cap)
{
    extern __shared__ int ctg_lds[];
    __shared__ unsigned long long wdrop[256 / kWave];
    ctg_stage(g, ix.n, ctg_lds);
    const int lane = threadIdx.x & (kWave - 1);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const LcRow q = lc_row(ix, rows, i, S);
    long long off = 0;
    if (FILL && i < S) off = offsets[i];
    const bool big = q.cnt > 32;
    int kept = 0, drop = 0;
    if (!big)
        for (int k = 0; k < q.cnt; k++) {
            int2 o;
            const int what = lc_hit(ix, g, ctg_lds, q.lo + k, q.len, o);
            if (what == 1) {
                if (FILL && off + kept < cap) hits[off + kept] = o;
                kept++;
            }
            drop += what == 2;
        }
    unsigned long long todo = __ballot(big);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int blo = __shfl(q.lo, src), bcnt = __shfl(q.cnt, src), blen = __shfl(q.len, src);
        const long long boff = __shfl(off, src);
        int seen = 0, gone = 0;
        for (int k0 = 0; k0 < bcnt; k0 += kWave) {               // wave-uniform trip count
            const int k = k0 + lane;
            int2 o = make_int2(0, 0);
            const int what = k < bcnt ? lc_hit(ix, g, ctg_lds, blo + k, blen, o) : 0;
            const unsigned long long mask = __ballot(what == 1);
            if (FILL && what == 1) {
                const long long at = boff + seen + __popcll(mask & ((1ull << lane) - 1ull));
                if (at < cap) hits[at] = o;
            }
            seen += __popcll(mask);
            gone += __popcll(__ballot(what == 2));
        }
        if (lane == src) { kept = seen; drop = gone; }
    }
    if (!FILL) {
        if (i < S) counts[i] = kept;
        // the block's dropped occurrences go to its own word: one atomicAdd per wave on a single word costs more than the
        // walk itself once most occurrences bridge (measured: DESIGN.md section 18)
        unsigned long long d = (unsigned long long)drop;
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) d += (unsigned long long)__shfl_xor((long long)d, o);
        if (lane == 0) wdrop[threadIdx.x / kWave] = d;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long all = 0;
            for (int w = 0; w < 256 / kWave; w++) all += wdrop[w];
            dropped[blockIdx.x] = all;
        }
    }
}

// {hits kept, occurrences dropped}: the sum of the blocks' words, by one block
__global__ void __launch_bounds__(256) lc_totals_kernel(const long long *__restrict__ offsets, long long S,
                                                        const unsigned long long *__restrict__ dropped, long long blocks,
                                                        long long *__restrict__ totals)
{
    __shared__ unsigned long long wsum[256 / kWave];
    unsigned long long d = 0;
    for (long long b = threadIdx.x; b < blocks; b += 256) d += dropped[b];
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) d += (unsigned long long)__shfl_xor((long long)d, o);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int w = 0; w < 256 / kWave; w++) all += wsum[w];
        totals[0] = offsets[S];
        totals[1] = (long long)all;
    }
}

struct LcArea {
    int32_t *counts;                      // hits kept per interval
    unsigned long long *dropped;          // one word per block of the walk
    uint8_t *scan_tmp;                    // launch_compact's scratch
};

inline int64_t lc_layout(uint8_t *base, int64_t S, LcArea *a)
{
    Carver c{base};
    c.take(a->counts, S * 4);
    c.take(a->dropped, 8 * ((S + 255) / 256));
    c.take(a->scan_tmp, compact_tmp_bytes(S));
    return c.at;
}

}  // namespace

int contigs_validate(const genie_index *ix, const int64_t *d_off, int64_t n_contigs, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    unsigned int *d_bad = nullptr, h_bad = 0;
    HIP_TRY(hipMalloc(&d_bad, sizeof(unsigned int)));
    hipError_t e = hipMemsetAsync(d_bad, 0, sizeof(unsigned int), s);
    if (e == hipSuccess) {
        const long long want = (n_contigs + 1 + 255) / 256, most = (long long)(ix->num_cus > 0 ? ix->num_cus : 256) * 8;
        hipLaunchKernelGGL(ctg_validate_kernel, dim3((unsigned)std::min(want, most)), dim3(256), 0, s,
                           reinterpret_cast<const long long *>(d_off), (long long)n_contigs, (long long)ix->dev.n, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, d_bad, sizeof(unsigned int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_bad);
    if (e != hipSuccess) { set_hip_error("contigs_validate", (int)e); return GENIE_E_HIP; }
    return h_bad ? GENIE_E_INVALID : GENIE_OK;
}

int launch_contig_coords(const genie_index *ix, const int64_t *d_off, int64_t n_contigs, const int32_t *d_pos, int32_t stride,
                         int64_t count, int32_t *d_out, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (count == 0) return GENIE_OK;
    const CtgTab g = ctg_tab(d_off, n_contigs);
    LAUNCH_BLOCKS(ctg_coords_kernel, (count + 255) / 256, 256, ctg_lds_bytes(g), s, ix->dev, g, d_pos, (int)stride, (long long)count,
                  d_out);
    return GENIE_OK;
}

int64_t locate_contigs_tmp_bytes(int64_t S)
{
    LcArea a;
    return lc_layout(nullptr, S, &a);
}

int launch_locate_contigs(const genie_index *ix, const int64_t *d_off, int64_t n_contigs, const int32_t *d_rows, int64_t S,
                          int64_t *d_hit_offsets, int32_t *d_hits, int64_t cap_hits, int64_t *d_totals, void *d_tmp, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (S == 0) {
        HIP_TRY(hipMemsetAsync(d_hit_offsets, 0, 8, s));
        if (d_totals) HIP_TRY(hipMemsetAsync(d_totals, 0, 16, s));
        return GENIE_OK;
    }
    LcArea a;
    lc_layout(static_cast<uint8_t *>(d_tmp), S, &a);
    const CtgTab g = ctg_tab(d_off, n_contigs);
    const int4 *rows = reinterpret_cast<const int4 *>(d_rows);
    dim3 grid;
    if (int rc = grid_for((S + 255) / 256, 256, &grid)) return rc;
    LAUNCH(lc_walk_kernel<false>, grid, dim3(256), ctg_lds_bytes(g), s, ix->dev, g, rows, (long long)S, a.counts, a.dropped,
           static_cast<const long long *>(nullptr), static_cast<int2 *>(nullptr), 0ll);
    int rc = launch_compact(a.counts, nullptr, S, 0x7FFFFFFF, d_hit_offsets, nullptr, 0, a.scan_tmp, stream);
    if (rc) return rc;
    if (d_totals)
        LAUNCH(lc_totals_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<const long long *>(d_hit_offsets), (long long)S,
               static_cast<const unsigned long long *>(a.dropped), (long long)((S + 255) / 256), reinterpret_cast<long long *>(d_totals));
    if (d_hits && cap_hits > 0)
        LAUNCH(lc_walk_kernel<true>, grid, dim3(256), ctg_lds_bytes(g), s, ix->dev, g, rows, (long long)S, a.counts, a.dropped,
               reinterpret_cast<const long long *>(d_hit_offsets), reinterpret_cast<int2 *>(d_hits), (long long)cap_hits);
    return GENIE_OK;
}

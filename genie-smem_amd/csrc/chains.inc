// chains.inc -- genie_chain_mems: the MEM rows of every strand-read chained into collinear chains (included by kernels.hip
// behind mems.inc, inside namespace genie).  The definition is the header's; DESIGN.md section 22 has the reasoning.
//
// A unit is one strand-read: the rows off[u] .. off[u+1) of the MEM CSR.  One wave owns a unit from its first kernel to its
// last store; no unit is split, no wave waits for another, every loop is bounded by a row count.
//   CH0 chain_check_kernel    off[0] == 0, non-decreasing, off[U] <= total_rows, no unit above 2^31 - 1 rows; the host reads
//                             the flag: the call's one synchronisation
//   CH1 chain_contig_kernel   only with more than one contig: the contig of every anchor (ctg_stage / ctg_find), one lane per row
//   CH2 chain_forward_kernel  per unit: the recurrence (f, p), then the tops, then the count of its chains
//        forward  anchors in row order, 64 to a chunk.  A chunk's rows are loaded by the wave, one per lane, and their
//                 (s, t, c, f) go into the wave's LDS ring of kChainTile anchors; anchor i's own values come out of the
//                 loading lane by v_readlane.  The 64 lanes go over the candidates j of the window -- s_j >= s_i - max_dist,
//                 cut by max_pred; contiguous because s is sorted, its start a pointer that only moves up -- one 16-byte LDS
//                 read each, and a wave max-reduce over (value, j) decides (f, p).  Candidates older than the ring are read
//                 from the rows and the workspace (L2).
//        tops     chunks in descending order.  key = (f, smaller index first); inside a chunk the keys move from child to
//                 parent by v_readlane, highest lane first; a parent below the chunk gets the key by a 64-bit atomic max into
//                 the workspace, which the chunk that holds it reads back.  max is order-free: no atomic decides a value.
//        count    one lane per leaf (top(i) == i) follows p while top == leaf: score, kept flag per row, chains per unit
//        A unit of at most 64 rows reads nothing back: (f, p) stay in the lanes, the leaves walk (p, top, f) in the ring.
//   scan          launch_compact over the units' counts writes d_chain_offsets (scan_block_sums_kernel)
//   CH3 chain_totals_kernel   {chains kept, chains not kept}
//   CH4 chain_fill_kernel     per unit: the rank of every kept leaf by ballots in row order; the leaf's lane walks its chain
//                             once more, writes the chain row and its members' d_anchor_chain: one lane per anchor
namespace {

constexpr int kChainTile = 512;           // anchors of a wave's LDS ring: a power of two in [64, 4096]
constexpr int kChainWaves = 4;            // waves per block: 4 x 512 x 16 bytes = 32 KB of LDS, five blocks per CU by LDS
static_assert((kChainTile & (kChainTile - 1)) == 0 && kChainTile >= 64 && kChainTile <= 4096, "kChainTile");
static_assert(2 * kChainWaves * kChainTile * 16 <= 160 * 1024, "two blocks per CU at least");

struct ChainParams {
    int max_dist, bandwidth, gap_cost, max_pred, min_score;
};

struct ChainArea {
    int *flag;                            // CH0's verdict
    int32_t *f, *p, *top, *keep;          // per row: score, predecessor, top of its chain, 1 on the top of a kept chain
    unsigned long long *tkey;             // per row: the largest key pushed up from chunks above
    int32_t *ctg;                         // per row, only with more than one contig
    int32_t *counts, *leaves;             // per unit: chains kept, chains in all
    uint8_t *scan_tmp;                    // launch_compact's scratch
};

inline int64_t chain_layout(uint8_t *base, int64_t U, int64_t R, bool with_ctg, ChainArea *a)
{
    Carver c{base};
    c.take(a->flag, 8);
    c.take(a->f, R * 4);
    c.take(a->p, R * 4);
    c.take(a->top, R * 4);
    c.take(a->keep, R * 4);
    c.take(a->tkey, R * 8);
    a->ctg = nullptr;
    if (with_ctg) c.take(a->ctg, R * 4);
    c.take(a->counts, U * 4);
    c.take(a->leaves, U * 4);
    c.take(a->scan_tmp, compact_tmp_bytes(U));
    return c.at;
}

__global__ void __launch_bounds__(256) chain_check_kernel(const long long *__restrict__ off, long long U, long long total,
                                                          int *__restrict__ flag)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > U) return;
    const long long o = off[r];
    bool bad = o < 0 || o > total || (r == 0 && o != 0);
    if (r < U) {
        const long long o2 = off[r + 1];
        bad = bad || o2 < o || o2 - o > 0x7fffffffll;
    }
    if (bad) atomicOr(flag, 1);
}

__global__ void __launch_bounds__(256) chain_contig_kernel(DevIndex ix, CtgTab g, const long long *__restrict__ off, long long U,
                                                           const int4 *__restrict__ rows, int32_t *__restrict__ ctg)
{
    extern __shared__ int ctg_lds[];
    ctg_stage(g, ix.n, ctg_lds);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= off[U]) return;
    ctg[i] = ctg_find(g, ctg_lds, ix.n, (int)((unsigned)rows[i].z - 1u)).c;
}

// (f, smaller index first) as one unsigned word; 0 is below every key
__device__ __forceinline__ unsigned long long chain_key(int f, int i)
{
    return ((unsigned long long)((unsigned)f ^ 0x80000000u) << 32) | (unsigned)(0x7fffffff - i);
}

__device__ __forceinline__ int chain_key_index(unsigned long long k) { return 0x7fffffff - (int)(unsigned)k; }

__device__ __forceinline__ unsigned long long chain_readlane64(unsigned long long v, int k)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), k);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long chain_wave_max64(unsigned long long v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, kWave);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, kWave);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

// The unit's arrays, all offset to its first row
struct ChainUnit {
    const int4 *rows;
    const int32_t *ctg;                   // or null: every contig is 0
    int32_t *f, *p, *top, *keep;
    unsigned long long *tkey;
    int n;
};

// One chain, from its top down to its first anchor: the lane of the leaf calls it.  mark (or null) gets `value` at every member.
struct ChainRow {
    int q_begin, q_end, r_begin, r_end, score, count;
};

__device__ __forceinline__ ChainRow chain_walk(const ChainUnit &u, int leaf, int32_t *__restrict__ mark, int value)
{
    ChainRow c{0, (int)0x80000000, 0, (int)0x80000000, 0, 0};
    int j = leaf;
    while (j >= 0 && c.count < u.n && u.top[j] == leaf) {            // j falls strictly: p(j) < j
        const int4 r = u.rows[j];
        const int re = (int)((unsigned)r.z + ((unsigned)r.y - (unsigned)r.x));
        c.q_end = r.y > c.q_end ? r.y : c.q_end;
        c.r_end = re > c.r_end ? re : c.r_end;
        c.q_begin = r.x;
        c.r_begin = r.z;
        if (mark) mark[j] = value;
        c.count++;
        j = u.p[j];
    }
    c.score = (int)((unsigned)u.f[leaf] - (j >= 0 ? (unsigned)u.f[j] : 0u));
    return c;
}

// forward, tops and count of one unit, by one wave; ring: its kChainTile (s, t, c, f) slots
__device__ __forceinline__ void chain_unit(const ChainUnit &u, const ChainParams &prm, int4 *__restrict__ ring, int lane,
                                           int32_t *__restrict__ out_pred, int32_t *__restrict__ out_score, int &n_kept, int &n_leaves)
{
    constexpr int kMask = kChainTile - 1;
    const int n = u.n;
    // ---- forward
    int wlo = 0;                                                     // first row of the window: it only moves up
    int myf = 0, myp = -1;                                           // (f, p) of the lane's anchor of the chunk
    for (int b = 0; b < n; b += kWave) {
        const int i = b + lane;
        int s = 0, t = 0, l = 0, c = 0;
        if (i < n) {
            const int4 r = u.rows[i];
            s = r.x;
            l = (int)((unsigned)r.y - (unsigned)r.x);
            t = (int)((unsigned)r.z - 1u);
            c = u.ctg ? u.ctg[i] : 0;
            ring[i & kMask] = make_int4(s, t, c, 0);
        }
        __builtin_amdgcn_wave_barrier();
        const int ring_lo = b + kWave - kChainTile;                  // the ring holds the rows from here on
        const int cnt = n - b < kWave ? n - b : kWave;
        for (int k = 0; k < cnt; k++) {
            const int ii = b + k;
            const int si = __builtin_amdgcn_readlane(s, k), ti = __builtin_amdgcn_readlane(t, k);
            const int li = __builtin_amdgcn_readlane(l, k), ci = __builtin_amdgcn_readlane(c, k);
            const long long s_min = (long long)si - prm.max_dist;
            while (wlo < ii) {                                       // at most one pass that does not move wlo per anchor
                const int j = wlo + lane;
                bool out = false;
                if (j < ii) out = (long long)(j >= ring_lo ? ring[j & kMask].x : u.rows[j].x) < s_min;
                const unsigned long long m = __ballot(out);
                const int adv = m == ~0ull ? kWave : __ffsll((long long)~m) - 1;
                wlo += adv;
                if (adv < kWave) break;
            }
            int lo = wlo;
            if (prm.max_pred > 0 && ii - prm.max_pred > lo) lo = ii - prm.max_pred;
            int f = li, p = -1;
            if (lo < ii) {
                int bv = (int)0x80000000, bj = -1;
                for (int j0 = lo; j0 < ii; j0 += kWave) {
                    const int j = j0 + lane;
                    if (j < ii) {
                        int4 a;
                        if (j >= ring_lo) {
                            a = ring[j & kMask];
                        } else {
                            const int4 r = u.rows[j];
                            a = make_int4(r.x, (int)((unsigned)r.z - 1u), u.ctg ? u.ctg[j] : 0, u.f[j]);
                        }
                        const unsigned dq = (unsigned)si - (unsigned)a.x, dr = (unsigned)ti - (unsigned)a.y;
                        if (a.z == ci && dq - 1u < (unsigned)prm.max_dist && dr - 1u < (unsigned)prm.max_dist) {
                            const unsigned g = dr > dq ? dr - dq : dq - dr;
                            int mn = li;
                            mn = (int)dq < mn ? (int)dq : mn;
                            mn = (int)dr < mn ? (int)dr : mn;
                            const int gain = mn - (int)((g * (unsigned)prm.gap_cost) >> 4);
                            const int v = (int)((unsigned)a.w + (unsigned)gain);
                            if (g <= (unsigned)prm.bandwidth && gain >= 1 && v >= bv) {      // a lane's j rise: >= keeps the largest
                                bv = v;
                                bj = j;
                            }
                        }
                    }
                }
                const unsigned long long best =
                    chain_wave_max64(((unsigned long long)((unsigned)bv ^ 0x80000000u) << 32) | (unsigned)(bj + 1));
                const int vmax = (int)((unsigned)(best >> 32) ^ 0x80000000u), jmax = (int)(unsigned)best - 1;
                if (jmax >= 0 && vmax > li) {
                    f = vmax;
                    p = jmax;
                }
            }
            if (lane == k) {
                myf = f;
                myp = p;
                ring[ii & kMask].w = f;
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (i < n) {
            u.f[i] = myf;
            u.p[i] = myp;
            if (n > kWave) u.tkey[i] = 0ull;
            if (out_score) out_score[i] = myf;
            if (out_pred) out_pred[i] = myp;
        }
        if (n > kChainTile) __threadfence();                         // candidates that leave the ring are read back from here
    }
    if (n <= kWave) {
        // One chunk, most units of short reads: (f, p) are still in the lanes, the tops move by v_readlane, and the leaves
        // walk (p, top, f) in the ring.  Nothing is read back from memory: the stores are for the fill kernel.
        unsigned long long key = lane < n ? chain_key(myf, lane) : 0ull;
        for (int k = n - 1; k >= 1; k--) {
            const int pp = __builtin_amdgcn_readlane(myp, k);
            if (pp >= 0) {                                           // wave-uniform
                const unsigned long long child = chain_readlane64(key, k);
                if (lane == pp && child > key) key = child;
            }
        }
        const int tp = chain_key_index(key);
        if (lane < n) ring[lane] = make_int4(myp, tp, myf, 0);
        __builtin_amdgcn_wave_barrier();
        const bool leaf = lane < n && tp == lane;
        bool keep = false;
        if (leaf) {
            int j = lane;
            while (j >= 0 && ring[j].y == lane) j = ring[j].x;       // j falls strictly: p(j) < j
            keep = (int)((unsigned)myf - (j >= 0 ? (unsigned)ring[j].z : 0u)) >= prm.min_score;
        }
        if (lane < n) {
            u.top[lane] = tp;
            u.keep[lane] = keep ? 1 : 0;
        }
        n_kept = __popcll(__ballot(keep));
        n_leaves = __popcll(__ballot(leaf));
        return;
    }
    __threadfence();                                                 // the wave reads back what its lanes stored
    // ---- tops
    const int last = (n - 1) & ~(kWave - 1);
    for (int b = last; b >= 0; b -= kWave) {
        const int i = b + lane;
        int pk = -1;
        unsigned long long key = 0;
        if (i < n) {
            pk = u.p[i];
            key = chain_key(u.f[i], i);
            if (b != last) {
                const unsigned long long up = __hip_atomic_load(&u.tkey[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                key = up > key ? up : key;
            }
        }
        const int cnt = n - b < kWave ? n - b : kWave;
        for (int k = cnt - 1; k >= 1; k--) {
            const int pp = __builtin_amdgcn_readlane(pk, k);
            if (pp >= b) {                                           // wave-uniform
                const unsigned long long child = chain_readlane64(key, k);
                if (lane == pp - b && child > key) key = child;
            }
        }
        if (i < n) {
            u.top[i] = chain_key_index(key);
            if (pk >= 0 && pk < b) atomicMax(&u.tkey[pk], key);
        }
        __threadfence();
    }
    // ---- count
    n_kept = 0;
    n_leaves = 0;
    for (int b = 0; b < n; b += kWave) {
        const int i = b + lane;
        bool leaf = false, keep = false;
        if (i < n && u.top[i] == i) {
            leaf = true;
            keep = chain_walk(u, i, nullptr, 0).score >= prm.min_score;
        }
        if (i < n) u.keep[i] = keep ? 1 : 0;
        n_kept += __popcll(__ballot(keep));
        n_leaves += __popcll(__ballot(leaf));
    }
}

__global__ void __launch_bounds__(kChainWaves *kWave) chain_forward_kernel(const long long *__restrict__ off, long long U,
                                                                            const int4 *rows, ChainArea a, ChainParams prm,
                                                                            int32_t *out_pred, int32_t *out_score)
{
    __shared__ int4 rings[kChainWaves][kChainTile];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (long long w = (long long)blockIdx.x * kChainWaves + wave; w < U; w += (long long)gridDim.x * kChainWaves) {
        const long long o = off[w];
        const ChainUnit u{rows + o, a.ctg ? a.ctg + o : nullptr, a.f + o, a.p + o, a.top + o, a.keep + o, a.tkey + o, (int)(off[w + 1] - o)};
        int kept = 0, leaves = 0;
        if (u.n > 0) chain_unit(u, prm, rings[wave], lane, out_pred ? out_pred + o : nullptr, out_score ? out_score + o : nullptr, kept, leaves);
        if (lane == 0) {
            a.counts[w] = kept;
            a.leaves[w] = leaves;
        }
    }
}

__global__ void __launch_bounds__(kChainWaves *kWave) chain_fill_kernel(const long long *__restrict__ off, long long U, const int4 *rows,
                                                                         ChainArea a, const long long *__restrict__ chain_off,
                                                                         int4 *__restrict__ chains, long long cap,
                                                                         int32_t *__restrict__ anchor_chain)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (long long w = (long long)blockIdx.x * kChainWaves + wave; w < U; w += (long long)gridDim.x * kChainWaves) {
        const long long o = off[w];
        const ChainUnit u{rows + o, a.ctg ? a.ctg + o : nullptr, a.f + o, a.p + o, a.top + o, a.keep + o, a.tkey + o, (int)(off[w + 1] - o)};
        const long long first = chain_off[w];
        int before = 0;                                              // kept chains of the unit in front of this chunk
        for (int b = 0; b < u.n; b += kWave) {
            const int i = b + lane;
            const bool keep = i < u.n && u.keep[i] != 0;
            const unsigned long long m = __ballot(keep);
            const int rank = before + __popcll(m & ((1ull << lane) - 1ull));
            before += __popcll(m);
            if (i < u.n && u.top[i] == i) {
                const ChainRow c = chain_walk(u, i, anchor_chain ? anchor_chain + o : nullptr, keep ? rank : -1);
                if (keep && chains && first + rank < cap) {
                    chains[2 * (first + rank)] = make_int4(c.q_begin, c.q_end, c.r_begin, c.r_end);
                    chains[2 * (first + rank) + 1] = make_int4(c.score, c.count, u.ctg ? u.ctg[i] : 0, i);
                }
            }
        }
    }
}

// {chains kept, chains not kept}, by one block
__global__ void __launch_bounds__(kScanBlock) chain_totals_kernel(const long long *__restrict__ chain_off, long long U,
                                                                  const int32_t *__restrict__ leaves, long long *__restrict__ totals)
{
    __shared__ unsigned long long wsum[kScanBlock / kWave];
    unsigned long long d = 0;
    for (long long w = threadIdx.x; w < U; w += kScanBlock) d += (unsigned long long)leaves[w];
    d = wave_sum64(d);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int w = 0; w < kScanBlock / kWave; w++) all += wsum[w];
        totals[0] = chain_off[U];
        totals[1] = (long long)all - chain_off[U];
    }
}

}  // namespace

int64_t chain_mems_workspace_bytes(int64_t U, int64_t total_rows, int64_t n_contigs)
{
    ChainArea a;
    return chain_layout(nullptr, U, total_rows, n_contigs > 1, &a);
}

int launch_chain_mems(const genie_index *ix, const ContigTable &ctg, const ChainBatch &b, const CsrRows &out, const ChainAnchors &an,
                      void *d_ws, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t U = b.U, R = b.total_rows;
    if (U == 0) {
        HIP_TRY(hipMemsetAsync(out.offsets, 0, 8, s));
        if (out.totals) HIP_TRY(hipMemsetAsync(out.totals, 0, 16, s));
        return GENIE_OK;
    }
    const bool with_ctg = ctg.n_contigs > 1;
    ChainArea a;
    chain_layout(static_cast<uint8_t *>(d_ws), U, R, with_ctg, &a);
    const long long *off = reinterpret_cast<const long long *>(b.offsets);
    const int4 *rows = reinterpret_cast<const int4 *>(b.rows);
    HIP_TRY(hipMemsetAsync(a.flag, 0, 8, s));
    LAUNCH_BLOCKS(chain_check_kernel, (U + 1 + 255) / 256, 256, 0, s, off, (long long)U, (long long)R, a.flag);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, a.flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return GENIE_E_INVALID;
    if (with_ctg && R > 0) {
        const CtgTab g = ctg_tab(ctg.offsets, ctg.n_contigs);
        LAUNCH_BLOCKS(chain_contig_kernel, (R + 255) / 256, 256, ctg_lds_bytes(g), s, ix->dev, g, off, (long long)U, rows, a.ctg);
    }
    const ChainParams prm{b.max_dist, b.bandwidth, b.gap_cost, b.max_pred, b.min_score};
    const long long want = (U + kChainWaves - 1) / kChainWaves, most = (long long)(ix->num_cus > 0 ? ix->num_cus : 256) * 4;
    const dim3 grid((unsigned)std::min(want, most));
    LAUNCH(chain_forward_kernel, grid, dim3(kChainWaves * kWave), 0, s, off, (long long)U, rows, a, prm, an.pred, an.score);
    int rc = launch_compact(a.counts, nullptr, U, 0x7FFFFFFF, out.offsets, nullptr, 0, a.scan_tmp, stream);
    if (rc) return rc;
    const long long *chain_off = reinterpret_cast<const long long *>(out.offsets);
    if (out.totals)
        LAUNCH(chain_totals_kernel, dim3(1), dim3(kScanBlock), 0, s, chain_off, (long long)U, static_cast<const int32_t *>(a.leaves),
               reinterpret_cast<long long *>(out.totals));
    if ((out.rows && out.cap_rows > 0) || an.chain)
        LAUNCH(chain_fill_kernel, grid, dim3(kChainWaves * kWave), 0, s, off, (long long)U, rows, a, chain_off,
               reinterpret_cast<int4 *>(out.rows), (long long)(out.rows ? out.cap_rows : 0), an.chain);
    return GENIE_OK;
}

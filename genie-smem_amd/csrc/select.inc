// select.inc -- genie_select_alignments: per read, which chains of genie_align_chains are its primary, supplementary and secondary
// alignments, with a mapping quality (included by align.inc behind cigars.inc, inside namespace genie).  The definition is the
// header's; DESIGN.md section 25 has the reasoning.
//
// The walk in key order is run as greedy rounds: the best unassigned candidate becomes a primary and takes every unassigned
// candidate that overlaps it as its secondary; the pass that hands them out also finds the best of those that stay unassigned,
// so a round is one pass over the read's chains.  The selected secondaries are min(max_secondary, eligible) further arg-max
// rounds.  No sort.  sel_run is that program once, for one lane alone or for the 64 lanes of a wave:
//   SE0 chain_check_kernel   the chain offsets; the host reads the flag: the call's one synchronisation
//   SE1 select_lane_kernel   one lane per read: marks the reads of more than kSelLaneMax chains as wide and runs the others,
//                            their state in d_class
//   SE2 launch_compact       the wide reads as a list (scan_block_sums_kernel)
//   SE3 select_wave_kernel   one wave per wide read, grid-stride over that list: lane l owns the chains l, l + 64, ...; their
//                            (score, interval, state) in LDS up to kSelTile chains, beyond it read back from d_aln and d_class
//   SE4 launch_compact       the reads' selected counts to d_sel_offsets
//   SE5 select_write_kernel  one lane per chain: a selected chain writes its d_sel entry and its record
//   SE6 select_totals_kernel the four totals, by one block
// A lane only ever reads the state of chains it owns; what the wave shares (the arg-max, the primary's interval, the sums) goes
// through shuffles.  Every round assigns at least its primary, so a read of n chains takes at most n rounds.
namespace {

constexpr int kSelLaneMax = GENIE_SELECT_LANE_MAX;            // a read of at most this many chains is run by one lane
constexpr int kSelTile = GENIE_SELECT_TILE;                   // chains of a wide read whose state lives in LDS
constexpr int kSelWaves = 4;                                  // waves per block
static_assert(kSelTile % kWave == 0 && 4 * kSelWaves * kSelTile * 16 <= 160 * 1024, "four blocks per CU");

// the state of a chain while its read is run; 0 .. 3 are the kinds of d_class
enum : int { kSelUnassigned = -1, kSelPrimary = 0, kSelSupp = 1, kSelSecondary = 2, kSelNone = 3, kSelPend = 5 };
constexpr int kSelPending = -2;                               // the order of an eligible secondary until the selection is made

struct SelParams {
    int mask_level, pri_ratio, max_secondary, min_score, mapq_full;
};

struct SelInput {
    const long long *roff;
    long long N;
    int S;
    const long long *coff;
    long long U;
    const int4 *chains, *aln;
    long long cap;
    const long long *ctg;                 // or null
    int nctg;
};

struct SelectArea {
    int *flag;                            // SE0's verdict
    int32_t *sub;                         // per chain: sub(P) of a primary
    int4 *counts;                         // per read: d_read_counts where the caller gives none
    int32_t *nsel, *wide;                 // per read: chains selected; 1 for a wide read
    int4 *wslot, *wlist;                  // per read: its index as a row, and the rows of the wide reads
    long long *woff;                      // N + 1
    uint8_t *scan_tmp;                    // launch_compact's
};

inline int64_t select_layout(uint8_t *base, int64_t N, int64_t cap_chains, SelectArea *a)
{
    Carver c{base};
    c.take(a->flag, 8);
    c.take(a->sub, cap_chains * 4);
    c.take(a->counts, N * 16);
    c.take(a->nsel, N * 4);
    c.take(a->wide, N * 4);
    c.take(a->wslot, N * 16);
    c.take(a->wlist, N * 16);
    c.take(a->woff, (N + 1) * 8);
    c.take(a->scan_tmp, compact_tmp_bytes(N));
    return c.at;
}

__device__ __forceinline__ long long sel_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ long long sel_chain_count(const SelInput &in)
{
    const long long total = in.coff[in.U];
    return total < in.cap ? (total < 0 ? 0 : total) : in.cap;
}

// the chains [lo, lo + n) of a read, those from mid on on strand 1, and its length
struct SelRead {
    int lo, n, mid, L;
};

__device__ __forceinline__ SelRead sel_read(const SelInput &in, long long i)
{
    const long long C = sel_chain_count(in);
    const long long a = sel_clamp(in.coff[in.S * i], 0, C), b = sel_clamp(in.coff[in.S * i + in.S], a, C);
    const long long m = in.S == 2 ? sel_clamp(in.coff[2 * i + 1], a, b) : b;
    return SelRead{(int)a, (int)(b - a), (int)m, (int)sel_clamp(in.roff[i + 1] - in.roff[i], 0, 0x7fffffffll)};
}

// [q_begin, q_end) of a strand-read in forward read coordinates, both ends clamped to [0, L]
__device__ __forceinline__ int2 sel_forward(int qb, int qe, bool rev, int L)
{
    const long long b = rev ? (long long)L - qe : qb, e = rev ? (long long)L - qb : qe;
    return make_int2((int)sel_clamp(b, 0, L), (int)sel_clamp(e, 0, L));
}

// (score, forward begin, forward end, is a candidate) of chain j of the read
__device__ __forceinline__ int4 sel_load(const SelInput &in, const SelParams &p, const SelRead &r, int j)
{
    const long long c = (long long)r.lo + j;
    const int4 a0 = in.aln[2 * c];
    const int flags = in.aln[2 * c + 1].y;
    const int2 f = sel_forward(a0.y, a0.z, (int)c >= r.mid, r.L);
    return make_int4(a0.x, f.x, f.y, ((flags & 4) == 0 && a0.x >= p.min_score) ? 1 : 0);
}

__device__ __forceinline__ bool sel_overlap(int b1, int e1, int b2, int e2, int mask_level)
{
    const long long lo = b1 > b2 ? b1 : b2, hi = e1 < e2 ? e1 : e2, ov = hi > lo ? hi - lo : 0;
    const long long l1 = (long long)e1 - b1, l2 = (long long)e2 - b2;
    return 100 * ov > (long long)mask_level * (l1 < l2 ? l1 : l2);
}

// (score descending, index ascending) as one unsigned word; a candidate's score is at least 1, so 0 is below every key
__device__ __forceinline__ unsigned long long sel_key(int score, int j)
{
    return ((unsigned long long)(unsigned)score << 32) | (unsigned)(0x7fffffff - j);
}

__device__ __forceinline__ int sel_mapq(int score, int sub, int matched, int full)
{
    const long long s = score, d = s - (sub < s ? sub : s), m = sel_clamp(matched, 0, full);
    return s > 0 ? (int)(60 * d * m / (s * full)) : 0;
}

// One read.  kWide: the 64 lanes of a wave, lane l owning the chains l, l + 64, ... and `tile` holding (score, begin, end,
// state) of the first min(n, kSelTile) of them; else one lane alone, every chain's state in d_class.
template <bool kWide>
__device__ __forceinline__ void sel_run(const SelInput &in, const SelParams &p, const SelRead &r, int lane, int4 *tile,
                                        int4 *__restrict__ klass, int32_t *__restrict__ sub_of, int4 *counts, int32_t *nsel)
{
    constexpr int step = kWide ? kWave : 1;
    const int first = kWide ? lane : 0;
    const int nt = kWide ? (r.n < kSelTile ? r.n : kSelTile) : 0;
    int32_t *kcol = reinterpret_cast<int32_t *>(klass);
    auto get = [&](int j) -> int4 {
        if (kWide && j < nt) return tile[j];
        int4 d = sel_load(in, p, r, j);
        const int4 k = klass[(long long)r.lo + j];
        d.w = (k.x == kSelSecondary && k.z == kSelPending) ? (int)kSelPend : k.x;
        return d;
    };
    // every chain of the read: a candidate or not, and the best candidate
    unsigned long long mine = 0;
    int mb = 0, me = 0, ncand = 0;
    for (int j = first; j < r.n; j += step) {
        int4 d = sel_load(in, p, r, j);
        if (d.w) {
            ncand++;
            const unsigned long long k = sel_key(d.x, j);
            if (k > mine) {
                mine = k;
                mb = d.y;
                me = d.z;
            }
        }
        d.w = d.w ? (int)kSelUnassigned : (int)kSelNone;
        if (kWide && j < nt) tile[j] = d;
        klass[(long long)r.lo + j] = make_int4(d.w, -1, -1, 0);
    }
    if (kWide) ncand = (int)wave_sum64((unsigned long long)ncand);
    // the primaries, in key order
    int nprim = 0, nsec = 0, npend = 0, best = -1;
    for (int round = 0; round < r.n; round++) {
        const unsigned long long top = kWide ? chain_wave_max64(mine) : mine;
        if (top == 0) break;
        const int P = 0x7fffffff - (int)(unsigned)top, ps = (int)(top >> 32), owner = P & (kWave - 1);
        const int pb = kWide ? __shfl(mb, owner, kWave) : mb, pe = kWide ? __shfl(me, owner, kWave) : me;
        mine = 0;
        int sub = 0;
        unsigned long long took = 0;                                 // secondaries << 32 | eligible ones
        for (int j = first; j < r.n; j += step) {
            const int4 d = get(j);
            if (d.w != kSelUnassigned || j == P) continue;
            if (sel_overlap(d.y, d.z, pb, pe, p.mask_level)) {
                const bool eligible = 100ll * d.x >= (long long)p.pri_ratio * ps;
                if (kWide && j < nt) tile[j].w = eligible ? (int)kSelPend : (int)kSelSecondary;
                klass[(long long)r.lo + j] = make_int4(kSelSecondary, r.lo + P, eligible ? kSelPending : -1, 0);
                sub = d.x > sub ? d.x : sub;
                took += (1ull << 32) | (eligible ? 1u : 0u);
            } else {
                const unsigned long long k = sel_key(d.x, j);
                if (k > mine) {
                    mine = k;
                    mb = d.y;
                    me = d.z;
                }
            }
        }
        if (kWide) {
            sub = aln_wave_max(sub);
            took = wave_sum64(took);
        }
        if (!kWide || lane == owner) {
            const int kind = nprim ? kSelSupp : kSelPrimary;
            const long long c = (long long)r.lo + P;
            if (kWide && P < nt) tile[P].w = kind;
            klass[c] = make_int4(kind, (int)c, nprim, sel_mapq(ps, sub, in.aln[2 * c + 1].w, p.mapq_full));
            sub_of[c] = sub;
        }
        if (nprim == 0) best = r.lo + P;
        nprim++;
        nsec += (int)(took >> 32);
        npend += (int)(unsigned)took;
    }
    // the selected secondaries: the best of the eligible ones, one per round
    const int want = p.max_secondary < npend ? p.max_secondary : npend;
    int taken = 0;
    for (; taken < want; taken++) {
        mine = 0;
        for (int j = first; j < r.n; j += step) {
            const int4 d = get(j);
            if (d.w != kSelPend) continue;
            const unsigned long long k = sel_key(d.x, j);
            mine = k > mine ? k : mine;
        }
        const unsigned long long top = kWide ? chain_wave_max64(mine) : mine;
        if (top == 0) break;
        const int P = 0x7fffffff - (int)(unsigned)top;
        if (!kWide || lane == (P & (kWave - 1))) {
            if (kWide && P < nt) tile[P].w = kSelSecondary;
            kcol[4 * ((long long)r.lo + P) + 2] = nprim + taken;
        }
    }
    if (npend > taken)                                               // the eligible ones that were left out
        for (int j = first; j < r.n; j += step)
            if (get(j).w == kSelPend) kcol[4 * ((long long)r.lo + j) + 2] = -1;
    if (!kWide || lane == 0) {
        *counts = make_int4(ncand, nprim, nsec, best);
        *nsel = nprim + taken;
    }
}

__global__ void __launch_bounds__(256) select_lane_kernel(SelInput in, SelParams p, int4 *__restrict__ klass, int32_t *__restrict__ sub_of,
                                                          int4 *__restrict__ counts, int32_t *__restrict__ nsel,
                                                          int32_t *__restrict__ wide, int4 *__restrict__ wslot)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.N) return;
    const SelRead r = sel_read(in, i);
    const bool w = r.n > kSelLaneMax;
    wide[i] = w ? 1 : 0;
    wslot[i] = make_int4((int)i, 0, 0, 0);
    if (w) return;                                                   // SE3 runs it
    sel_run<false>(in, p, r, 0, nullptr, klass, sub_of, counts + i, nsel + i);
}

__global__ void __launch_bounds__(kSelWaves *kWave) select_wave_kernel(SelInput in, SelParams p, const long long *__restrict__ woff,
                                                                        const int4 *__restrict__ wlist, int4 *__restrict__ klass,
                                                                        int32_t *__restrict__ sub_of, int4 *__restrict__ counts,
                                                                        int32_t *__restrict__ nsel)
{
    __shared__ int4 tiles[kSelWaves][kSelTile];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long long nw = sel_clamp(woff[in.N], 0, in.N);
    for (long long k = (long long)blockIdx.x * kSelWaves + wave; k < nw; k += (long long)gridDim.x * kSelWaves) {
        const long long i = sel_clamp(wlist[k].x, 0, in.N - 1);
        const SelRead r = sel_read(in, i);
        sel_run<true>(in, p, r, lane, tiles[wave], klass, sub_of, counts + i, nsel + i);
    }
}

__global__ void __launch_bounds__(256) select_write_kernel(SelInput in, const int4 *__restrict__ klass, const int32_t *__restrict__ sub_of,
                                                           const long long *__restrict__ sel_off, long long *__restrict__ sel,
                                                           int4 *__restrict__ records, long long cap_sel)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= sel_chain_count(in)) return;
    const int4 k = klass[c];
    if (k.z < 0) return;
    long long lo = 0, hi = in.U;                                     // the last u in [0, U) with coff[u] <= c
    while (lo < hi - 1) {
        const long long mid = (lo + hi) >> 1;
        if (in.coff[mid] <= c) lo = mid; else hi = mid;
    }
    const long long i = in.S == 2 ? lo >> 1 : lo;
    const int strand = in.S == 2 ? (int)(lo & 1) : 0;
    const long long pos = sel_off[i] + k.z;
    if (pos < 0 || pos >= cap_sel) return;
    const int4 a0 = in.aln[2 * c], a1 = in.aln[2 * c + 1];
    const int L = (int)sel_clamp(in.roff[i + 1] - in.roff[i], 0, 0x7fffffffll);
    const int2 f = sel_forward(a0.y, a0.z, strand != 0, L);
    int g = 0, offset = a0.w;
    if (in.ctg) {
        const int z = in.chains[2 * c + 1].z;
        g = z < 0 ? 0 : (z > in.nctg - 1 ? in.nctg - 1 : z);
        offset = (int)((long long)a0.w - in.ctg[g]);
    }
    sel[pos] = c;
    records[3 * pos] = make_int4((int)i, (int)c, k.x, strand);
    records[3 * pos + 1] = make_int4(g, offset, (int)((unsigned)a1.x - (unsigned)a0.w), f.x);
    records[3 * pos + 2] = make_int4(f.y, a0.x, k.x < kSelSecondary ? sub_of[c] : 0, k.w);
}

// {candidates, primaries, secondaries, selected}, by one block
__global__ void __launch_bounds__(kScanBlock) select_totals_kernel(const int4 *__restrict__ counts, long long N,
                                                                   const long long *__restrict__ sel_off, long long *__restrict__ totals)
{
    __shared__ unsigned long long wsum[3][kScanBlock / kWave];
    unsigned long long a = 0, b = 0, c = 0;
    for (long long i = threadIdx.x; i < N; i += kScanBlock) {
        const int4 v = counts[i];
        a += (unsigned long long)v.x;
        b += (unsigned long long)v.y;
        c += (unsigned long long)v.z;
    }
    a = wave_sum64(a);
    b = wave_sum64(b);
    c = wave_sum64(c);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        wsum[0][threadIdx.x / kWave] = a;
        wsum[1][threadIdx.x / kWave] = b;
        wsum[2][threadIdx.x / kWave] = c;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long all = 0;
        for (int w = 0; w < kScanBlock / kWave; w++) all += wsum[threadIdx.x][w];
        totals[threadIdx.x] = (long long)all;
    }
    if (threadIdx.x == 3) totals[3] = sel_off[N];
}

}  // namespace

int64_t select_alignments_workspace_bytes(int64_t N, int64_t cap_chains)
{
    SelectArea a;
    return select_layout(nullptr, N, cap_chains, &a);
}

int launch_select_alignments(const genie_index *ix, const ContigTable &ctg, const SelectBatch &b, const SelectOut &out, void *ws,
                             void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = b.N, U = b.U, cap = b.cap_chains;
    if (U == 0) {
        HIP_TRY(hipMemsetAsync(out.sel_offsets, 0, 8, s));
        if (out.totals) HIP_TRY(hipMemsetAsync(out.totals, 0, 32, s));
        return GENIE_OK;
    }
    SelectArea a;
    select_layout(static_cast<uint8_t *>(ws), N, cap, &a);
    const long long *coff = reinterpret_cast<const long long *>(b.chain_offsets);
    HIP_TRY(hipMemsetAsync(a.flag, 0, 8, s));
    LAUNCH_BLOCKS(chain_check_kernel, (U + 1 + 255) / 256, 256, 0, s, coff, (long long)U, 0x7fffffffffffffffll, a.flag);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, a.flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return GENIE_E_INVALID;
    const SelInput in{reinterpret_cast<const long long *>(b.read_offsets), (long long)N, b.S, coff, (long long)U,
                      reinterpret_cast<const int4 *>(b.chains), reinterpret_cast<const int4 *>(b.aln), (long long)cap,
                      ctg.n_contigs > 0 ? reinterpret_cast<const long long *>(ctg.offsets) : nullptr, (int)ctg.n_contigs};
    const SelParams p{b.mask_level, b.pri_ratio, b.max_secondary, b.min_score, b.mapq_full};
    int4 *klass = reinterpret_cast<int4 *>(out.klass);
    int4 *counts = out.read_counts ? reinterpret_cast<int4 *>(out.read_counts) : a.counts;
    LAUNCH_BLOCKS(select_lane_kernel, (N + 255) / 256, 256, 0, s, in, p, klass, a.sub, counts, a.nsel, a.wide, a.wslot);
    const long long wide_most = std::min<long long>(N, cap / (kSelLaneMax + 1));      // a wide read has more than kSelLaneMax chains
    if (wide_most > 0) {
        if (int rc = launch_compact(a.wide, reinterpret_cast<const int32_t *>(a.wslot), N, 1, reinterpret_cast<int64_t *>(a.woff),
                                    reinterpret_cast<int32_t *>(a.wlist), N, a.scan_tmp, stream))
            return rc;
        const long long want = (wide_most + kSelWaves - 1) / kSelWaves, most = (long long)(ix->num_cus > 0 ? ix->num_cus : 256) * 4;
        LAUNCH(select_wave_kernel, dim3((unsigned)std::min(want, most)), dim3(kSelWaves * kWave), 0, s, in, p,
               static_cast<const long long *>(a.woff), static_cast<const int4 *>(a.wlist), klass, a.sub, counts, a.nsel);
    }
    if (int rc = launch_compact(a.nsel, nullptr, N, 0x7FFFFFFF, out.sel_offsets, nullptr, 0, a.scan_tmp, stream)) return rc;
    const long long *sel_off = reinterpret_cast<const long long *>(out.sel_offsets);
    if (out.sel && out.cap_sel > 0 && cap > 0)
        LAUNCH_BLOCKS(select_write_kernel, (cap + 255) / 256, 256, 0, s, in, static_cast<const int4 *>(klass),
                      static_cast<const int32_t *>(a.sub), sel_off, reinterpret_cast<long long *>(out.sel),
                      reinterpret_cast<int4 *>(out.records), (long long)out.cap_sel);
    if (out.totals)
        LAUNCH(select_totals_kernel, dim3(1), dim3(kScanBlock), 0, s, static_cast<const int4 *>(counts), (long long)N, sel_off,
               reinterpret_cast<long long *>(out.totals));
    return GENIE_OK;
}

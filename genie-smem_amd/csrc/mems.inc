// mems.inc -- genie_find_mems: every maximal exact match (MEM) of at least min_len bases of every strand-read, with its
// reference position (included by kernels.hip behind long_units.inc, inside namespace genie).
//
// The call stands on the matching statistics: launch_match_stats, as it is, writes ms[v] and lohi[v] of every virtual
// position v (long_units.inc) into this call's workspace.  A position p of a strand-read Q with ms >= m = min_len has MEMs
// starting there; they are the left-maximal occurrences of the seed Q[p .. p+m).  What follows never reads the read again
// except for the one base in front of p:
//   the seed's rows   Q[p .. p+ms) equals the reference at s0 = SA[lohi.lo], so a row holds the seed iff its suffix shares
//                     m bases with the suffix s0: a comparison of the reference with itself;
//   a row's length    a row of lohi[v] has l = ms.  Any other row of the seed has l < ms (else it would lie in lohi[v]), so
//                     its match with Q ends inside Q[p .. p+ms) = T[s0 .. s0+ms): l = the longest common prefix of the
//                     suffixes t and s0, capped by the reference's end -- a break or the read's end cannot come first.
//   MEM1 mem_seed_kernel    one lane per virtual position, 256-position windows.  Where ms >= m: the inclusive rows I_m of
//                           the seed -- lohi itself when ms == m; two directory reads when m <= P; else lohi widened outward by
//                           two bounded searches inside the directory bucket of s0's P-mer (a gallop from lohi, then a
//                           bisection, both sides in step), each probe the row's inline 32-base key against that of row
//                           lohi.lo, the packed reference only past P + 32 bases.  max_occ is applied here (the position is
//                           dropped and counted).  Also the position inside its strand-read (mem_find) and the base in front
//                           of it (4: none, or a break).  One byte per position, prev[], tells the walks whether rows start
//                           there (kMemNone: not); everything else is written, and later read, for those positions alone --
//                           on a batch where few positions qualify the kernels are bound by the bytes they move per position.
//   MEM2 mem_walk_kernel<false>  counts, for every kept position, the rows of I_m whose occurrence is left-maximal (p == 0, t == 0
//                           or T[t-1] differs from the base in front): one lane per position up to kMemLaneRows rows, wider
//                           intervals by the whole wave in a ballot loop (locate_scatter_kernel's shape).  Blocks of kMemWalk
//                           positions; a block scans its counts in 64 bits: every kept position's offset inside its block,
//                           the block's sum, and per wave the mask of its kept positions.
//   scan_block_sums_kernel  over the block sums (one block: its time is the number of sums, hence the large walk blocks)
//   MEM3 mem_offsets_kernel a strand-read's offset is that of its first virtual position; the two totals
//   MEM4 mem_walk_kernel<true>   the same walk; the k-th left-maximal row of a position goes to offset + k as one 16-byte store
//                           while that is below out_cap_rows.  Rows of a position are in row order, positions in their own
//                           order: no atomic decides a value (one integer atomicAdd per block sums the skipped positions).
// Kernels of one block per window are launched in slices (LAUNCH_SLICED), as lr_ms_kernel is.
// genie_find_mems_contigs (a reference of several sequences, contigs.inc) is the same call with the CONTIGS instances of the
// walks: per occurrence one lookup of t in the contig table; an occurrence with less room than m to its contig's end is no
// row, a contig start is a left end, and a row's length is clipped to the room.  MEM1, the scan and MEM3 do not change.
namespace {

constexpr int kMemWin = 256;              // virtual positions per block
constexpr int kMemLaneRows = 32;          // a seed interval of more rows is walked by the whole wave
constexpr int kMemWalk = 1024;            // virtual positions per block of the walks: a quarter of the sums to scan
constexpr uint32_t kMemNone = 255;        // prev[] of a position where no row starts

struct MemArea {
    int32_t *ms;                          // S total
    uint8_t *prev;                        // S total: the base in front (strand order), 4 = none; kMemNone: no rows start here
    int2 *lohi, *seed;                    // S total each; seed, pos and pre are defined where rows start
    int32_t *pos;                         // S total: position inside the strand-read
    unsigned long long *pre;              // S total: rows of the walk block's positions in front
    unsigned long long *kept;             // one word per 64 positions: the positions where rows start
    unsigned long long *bsum;             // walk blocks + 1
    unsigned long long *skipped;          // one word
    uint8_t *stats;                       // launch_match_stats's workspace
    long long nwin, nwalk;                // blocks of MEM1, of the walks
};

inline int64_t mem_layout(uint8_t *base, int64_t N, int64_t total, int32_t flags, MemArea *a)
{
    const int64_t positions = ((flags & GENIE_READS_BOTH_STRANDS) ? 2 : 1) * total;
    a->nwin = (positions + kMemWin - 1) / kMemWin;
    a->nwalk = (positions + kMemWalk - 1) / kMemWalk;
    Carver c{base};
    c.take(a->ms, 4 * positions);
    c.take(a->lohi, 8 * positions);
    c.take(a->seed, 8 * positions);
    c.take(a->pos, 4 * positions);
    c.take(a->prev, positions);
    c.take(a->pre, 8 * positions);
    c.take(a->kept, 8 * a->nwalk * (kMemWalk / kWave));
    c.take(a->bsum, 8 * (a->nwalk + 1));
    c.take(a->skipped, 8);
    c.take(a->stats, match_stats_workspace_bytes(N, total, flags));
    return c.at;
}

// base t of the reference: one 8-byte load
__device__ __forceinline__ uint32_t mem_ref_base(const DevIndex &ix, int t)
{
    const uint64_t w = reinterpret_cast<const uint64_t *>(ix.ref)[(long long)(t >> 5) * 2];
    return (uint32_t)(w >> (62 - 2 * (t & 31))) & 3u;
}

// LuReads::find for one lane per position: the strand-read that holds virtual position v, i.e. the last q with at(q) <= v.
// The bisection over all strand-reads is a chain of log2(S N) dependent loads in every lane (twenty at 10^6 reads, the
// longest chain of MEM1); reads of similar lengths put the answer next to v / positions of the way through, so start there,
// gallop outward until two strand-reads bracket v and bisect between them: two or three probes on such a batch, and
// 2 log2(distance) on any other.
__device__ __forceinline__ long long mem_find(const LuReads &R, long long v, long long positions)
{
    const long long n = R.count();
    long long g = (long long)((double)v / (double)positions * (double)n);
    g = g < 0 ? 0 : (g > n - 1 ? n - 1 : g);
    long long lo, hi;                                            // at(lo) <= v or lo == 0; at(hi) > v or hi == n
    if (R.at(g) <= v) {
        lo = g;
        hi = g + 1;
        for (long long step = 1; hi < n && R.at(hi) <= v; step <<= 1) {
            lo = hi;
            hi = lo + 2 * step;
        }
        hi = hi < n ? hi : n;
    } else {
        hi = g;
        lo = g - 1;
        for (long long step = 1; lo > 0 && R.at(lo) > v; step <<= 1) {
            hi = lo;
            lo = hi - 2 * step;
        }
        lo = lo > 0 ? lo : 0;
    }
    while (lo < hi - 1) {
        const long long mid = (lo + hi) >> 1;
        if (R.at(mid) <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// Does the suffix of the row `rec` share its first m bases (m > P) with the suffix s0, whose inline key is key0?  The row
// lies in the directory bucket of s0's P-mer, so the first P bases are equal once the suffix has them.
__device__ __forceinline__ bool mem_row_has_seed(const DevIndex &ix, const SaRec rec, int m, int s0, uint64_t key0)
{
    if (ix.n - rec.s < m) return false;                         // runs off the reference: the key's zero padding is no base
    const int kb = m - ix.P;
    const uint64_t x = rec.key ^ key0;
    if (kb <= 32) return (x >> (64 - 2 * kb)) == 0;
    if (x) return false;
    for (int j = ix.P + 32; j < m; j += 32) {
        const uint64_t y = rwin(ix.ref, rec.s + j) ^ rwin(ix.ref, s0 + j);
        const int rem = m - j;
        if (rem < 32) return (y >> (64 - 2 * rem)) == 0;
        if (y) return false;
    }
    return true;
}

// MEM1
__global__ void __launch_bounds__(kMemWin) mem_seed_kernel(DevIndex ix, LuReads R, long long positions, int m, int max_occ,
                                                           const int32_t *__restrict__ ms, const int2 *__restrict__ lohi,
                                                           int2 *__restrict__ seed, int32_t *__restrict__ pos,
                                                           uint8_t *__restrict__ prev, unsigned long long *__restrict__ skipped,
                                                           long long win0)
{
    const long long v = (win0 + blockIdx.x) * kMemWin + threadIdx.x;
    int2 iv = make_int2(-1, -1);
    int p = 0;
    uint32_t pc = 4;
    bool skip = false;
    const int l = v < positions ? ms[v] : 0;
    if (l >= m) {
        const int2 lh = lohi[v];
        const LuSr sr = lu_sr(R, mem_find(R, v, positions));
        const long long pl = v - sr.at;
        if (lh.x >= 0 && lh.y >= lh.x && lh.y <= ix.n && pl >= 0 && pl < sr.o2 - sr.o) {
            p = (int)pl;
            if (p > 0) {
                const uint32_t c = R.bases[sr.rev ? sr.o2 - p : sr.o + p - 1];
                pc = c < 4u ? (sr.rev ? c ^ 3u : c) : 4u;
            }
            iv = lh;
            if (l > m) {
                const SaRec r0 = load_rec(ix.sa, lh.x);
                const uint64_t w = rwin(ix.ref, r0.s);
                if (m <= ix.P) {
                    const uint32_t code = (uint32_t)(w >> (64 - 2 * m));
                    iv = make_int2((int)dir_lb(ix, ix.dir, code, m), (int)dir_ub(ix, ix.dir, code, m) - 1);
                } else {
                    const uint32_t b = (uint32_t)(w >> (64 - 2 * ix.P));
                    // The first row that holds the seed lies in [lo1, hi1] and row hi1 holds it; the last one in [lo2, hi2] and
                    // row lo2 holds it.  Most seeds end within a row or two of lohi: gallop outward from it (step 1, 2, 4 ...),
                    // bisect once a row without the seed bounds the range (step 0); both sides probe in the same round,
                    // so that their rows are in flight together and a round costs one trip to memory, not two.
                    int lo1 = (int)ix.dir[b], hi1 = lh.x, lo2 = lh.y, hi2 = (int)dir_ub(ix, ix.dir, b, ix.P) - 1;
                    int st1 = 1, st2 = 1;
                    while (lo1 < hi1 || lo2 < hi2) {
                        const bool g1 = lo1 < hi1, g2 = lo2 < hi2;
                        const int d1 = hi1 - lo1, d2 = hi2 - lo2;    // a side that is done (d == 0) probes the row it knows
                        const int m1 = st1 ? hi1 - (st1 < d1 ? st1 : d1) : lo1 + (d1 >> 1);
                        const int m2 = st2 ? lo2 + (st2 < d2 ? st2 : d2) : lo2 + ((d2 + 1) >> 1);
                        const SaRec c1 = load_rec(ix.sa, m1), c2 = load_rec(ix.sa, m2);
                        const bool h1 = mem_row_has_seed(ix, c1, m, r0.s, r0.key), h2 = mem_row_has_seed(ix, c2, m, r0.s, r0.key);
                        if (g1) {
                            if (h1) { hi1 = m1; st1 = st1 < (1 << 29) ? st1 << 1 : st1; } else { lo1 = m1 + 1; st1 = 0; }
                        }
                        if (g2) {
                            if (h2) { lo2 = m2; st2 = st2 < (1 << 29) ? st2 << 1 : st2; } else { hi2 = m2 - 1; st2 = 0; }
                        }
                    }
                    iv = make_int2(hi1, lo2);
                }
            }
            if (max_occ > 0 && iv.y - iv.x >= max_occ) {
                skip = true;
                iv = make_int2(-1, -1);
            }
        }
    }
    // one byte per position tells the walks whether rows start there; the rest is written and read for those alone
    if (v < positions) {
        prev[v] = (uint8_t)(iv.x >= 0 ? pc : kMemNone);
        if (iv.x >= 0) {
            seed[v] = iv;
            pos[v] = p;
        }
    }
    const int nskip = __syncthreads_count(skip);
    if (threadIdx.x == 0 && nskip) atomicAdd(skipped, (unsigned long long)nskip);
}

// What a lane needs of its position to walk the seed's rows
struct MemPos {
    int lo, cnt;                          // first row and rows of the seed
    int llo, lhi;                         // lohi of the position: these rows match ms bases
    int ms, m, p;
    uint32_t pc;                          // base in front, 4 = none
};

// Is the occurrence at row r left-maximal?  Its start (0-based) goes to t.  CONTIGS: its room (the bases from t to the end
// of its contig) goes to room; an occurrence with less room than m is no row at all, and a contig start is a left end.
template <bool CONTIGS>
__device__ __forceinline__ bool mem_left_maximal(const DevIndex &ix, const CtgTab &cg, const int *__restrict__ cs, int m, int r,
                                                 uint32_t pc, int &t, int &room)
{
    t = ix.sa[r].s;
    if (CONTIGS) {
        const CtgHit h = ctg_find(cg, cs, ix.n, t);
        room = h.room;
        if (room < m) return false;
        return pc > 3u || t == 0 || t == h.start || mem_ref_base(ix, t - 1) != pc;
    }
    return pc > 3u || t == 0 || mem_ref_base(ix, t - 1) != pc;
}

// The row (start, end, pos, row) of a left-maximal occurrence; s0 = the start of row llo, loaded on first use (-1: not yet).
// CONTIGS: the length is clipped to room >= m.
template <bool CONTIGS>
__device__ __forceinline__ int4 mem_row(const DevIndex &ix, const MemPos &q, int r, int t, int &s0, int room)
{
    int l = q.ms;
    if (r < q.llo || r > q.lhi) {
        if (s0 < 0) s0 = ix.sa[q.llo].s;
        const int far = ix.n - (t > s0 ? t : s0);
        int lim = far < q.ms ? far : q.ms;
        if (CONTIGS) lim = lim < room ? lim : room;
        l = q.m;
        while (l < lim) {
            const uint64_t x = rwin(ix.ref, t + l) ^ rwin(ix.ref, s0 + l);
            if (x) { l += __clzll((long long)x) >> 1; break; }
            l += 32;
        }
        l = l < lim ? l : lim;
    } else if (CONTIGS) {
        l = l < room ? l : room;
    }
    return make_int4(q.p, q.p + l, t + 1, r);
}

// MEM2 (FILL false) / MEM4
template <bool FILL, bool CONTIGS>
__global__ void __launch_bounds__(kMemWalk) mem_walk_kernel(DevIndex ix, CtgPair cgs, long long positions, int m, const int32_t *__restrict__ ms,
                                                            const int2 *__restrict__ lohi, const int2 *__restrict__ seed,
                                                            const int32_t *__restrict__ pos, const uint8_t *__restrict__ prev,
                                                            unsigned long long *__restrict__ pre, unsigned long long *__restrict__ kept,
                                                            unsigned long long *__restrict__ bsum, int4 *__restrict__ rows,
                                                            long long cap, long long win0)
{
    __shared__ unsigned long long wtot[kMemWalk / kWave];
    extern __shared__ int ctg_lds[];                             // CONTIGS: the staged samples of the contig table
    __shared__ unsigned int ctg_occ;                             // CONTIGS: the seed rows of the block's positions (saturating)
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const long long win = win0 + blockIdx.x, v = win * kMemWalk + threadIdx.x;
    MemPos q{0, 0, 0, -1, 0, m, 0, 4u};
    long long off = 0;
    const uint32_t pc = v < positions ? prev[v] : kMemNone;
    if (pc != kMemNone) {
        const int2 iv = seed[v];
        q.lo = iv.x;
        q.cnt = iv.y - iv.x + 1;
        q.pc = pc;
        if (FILL) {
            const int2 lh = lohi[v];
            q.llo = lh.x;
            q.lhi = lh.y;
            q.ms = ms[v];
            q.p = pos[v];
            off = (long long)(bsum[win] + pre[v]);
        }
    }
    // CONTIGS.  Staging costs a block one load per sample, a lookup one load per level left below the samples.  Where the
    // table has more entries than the small staging holds (4 KB), a block whose positions have at least as many seed rows as
    // the large staging has samples takes that one (up to 48 KB), any other the small one, and a block without seed rows
    // none.  Count and fill see the same rows and choose alike.  A smaller table is staged whole, without the count.
    CtgTab cg = cgs.small;
    if (CONTIGS) {
        unsigned int occ = 1;
        if (cgs.big.ns != cgs.small.ns) {
            if (threadIdx.x == 0) ctg_occ = 0;
            __syncthreads();
            occ = (unsigned int)(q.cnt < (1 << 20) ? q.cnt : (1 << 20));
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1) occ += (unsigned int)__shfl_xor((int)occ, o);
            if (lane == 0 && occ) atomicAdd(&ctg_occ, occ);      // an integer sum: any order gives the same value
            __syncthreads();
            occ = ctg_occ;
            if (occ >= (unsigned int)cgs.big.ns) cg = cgs.big;
        }
        if (occ) ctg_stage(cg, ix.n, ctg_lds);
    }
    const bool wide = q.cnt > kMemLaneRows;
    unsigned long long n = 0;
    if (!wide) {
        int s0 = -1;
        for (int i = 0; i < q.cnt; i++) {
            int t, room = 0;
            if (!mem_left_maximal<CONTIGS>(ix, cg, ctg_lds, m, q.lo + i, q.pc, t, room)) continue;
            if (FILL && off + (long long)n < cap) rows[off + (long long)n] = mem_row<CONTIGS>(ix, q, q.lo + i, t, s0, room);
            n++;
        }
    }
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        MemPos b;
        b.lo = __shfl(q.lo, src);
        b.cnt = __shfl(q.cnt, src);
        b.pc = (uint32_t)__shfl((int)q.pc, src);
        b.m = m;
        long long boff = 0;
        if (FILL) {
            b.llo = __shfl(q.llo, src);
            b.lhi = __shfl(q.lhi, src);
            b.ms = __shfl(q.ms, src);
            b.p = __shfl(q.p, src);
            boff = __shfl(off, src);
        }
        unsigned long long seen = 0;
        int s0 = -1;
        for (int i0 = 0; i0 < b.cnt; i0 += kWave) {              // wave-uniform trip count
            const int i = i0 + lane;
            int t = 0, room = 0;
            const bool lm = i < b.cnt && mem_left_maximal<CONTIGS>(ix, cg, ctg_lds, m, b.lo + i, b.pc, t, room);
            const unsigned long long mask = __ballot(lm);
            if (FILL && lm) {
                const long long at = boff + (long long)seen + __popcll(mask & ((1ull << lane) - 1ull));
                if (at < cap) rows[at] = mem_row<CONTIGS>(ix, b, b.lo + i, t, s0, room);
            }
            seen += (unsigned long long)__popcll(mask);
        }
        if (lane == src) n = seen;
    }
    if (!FILL) {
        const unsigned long long inc = wave_inclusive_scan64(n, lane);
        if (lane == kWave - 1) wtot[wave] = inc;
        __syncthreads();
        unsigned long long before = inc - n, all = 0;
        for (int w = 0; w < kMemWalk / kWave; w++) {
            const unsigned long long x = wtot[w];
            before += w < wave ? x : 0ull;
            all += x;
        }
        const unsigned long long here = __ballot(pc != kMemNone);
        if (lane == 0) kept[v / kWave] = here;
        if (pc != kMemNone) pre[v] = before;
        if (threadIdx.x == 0) bsum[win] = all;
    }
}

// MEM3: bsum scanned (bsum[nwalk] = all rows).  pre[] is defined where rows start: the rows in front of a strand-read's
// first position are those in front of the next such position of its walk block (kept[]: at most kMemWalk / 64 words to
// look at), or all the block's when there is none.
__global__ void __launch_bounds__(256) mem_offsets_kernel(LuReads R, long long positions, long long nwalk,
                                                          const unsigned long long *__restrict__ kept,
                                                          const unsigned long long *__restrict__ pre,
                                                          const unsigned long long *__restrict__ bsum,
                                                          const unsigned long long *__restrict__ skipped,
                                                          long long *__restrict__ offsets, long long *__restrict__ totals)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > R.count()) return;
    const long long v = R.at(q);
    unsigned long long o = bsum[nwalk];
    if (v < positions) {
        const long long win = v / kMemWalk, wend = (win + 1) * (kMemWalk / kWave);
        long long w = v / kWave, u = v;
        unsigned long long mask = kept[w] >> (v & (kWave - 1));
        while (!mask && ++w < wend) {
            mask = kept[w];
            u = w * kWave;
        }
        o = mask ? bsum[win] + pre[u + __ffsll((long long)mask) - 1] : bsum[win + 1];
    }
    offsets[q] = (long long)o;
    if (q == 0 && totals) {
        totals[0] = (long long)bsum[nwalk];
        totals[1] = (long long)*skipped;
    }
}

}  // namespace

int64_t find_mems_workspace_bytes(int64_t N, int64_t total_bases, int32_t flags)
{
    MemArea a;
    return mem_layout(nullptr, N, total_bases, flags, &a);
}

// cg == nullptr: genie_find_mems; else genie_find_mems_contigs, whose walks run the CONTIGS instances
static int find_mems_any(const genie_index *ix, const CtgPair *cg, const CsrBatch &b, int32_t min_len, int32_t max_occ, const CsrRows &out,
                         void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (b.N == 0) {
        HIP_TRY(hipMemsetAsync(out.offsets, 0, 8, s));
        if (out.totals) HIP_TRY(hipMemsetAsync(out.totals, 0, 16, s));
        return GENIE_OK;
    }
    const long long positions = b.positions();
    MemArea a;
    const int64_t used = mem_layout(static_cast<uint8_t *>(b.ws), b.N, b.total_bases, b.flags, &a);
    // the matching statistics of the same batch into this call's workspace; what the caller gave beyond `used` is theirs too
    CsrBatch stats = b;
    stats.ws = a.stats;
    stats.ws_bytes = b.ws_bytes - (used - ws_align(match_stats_workspace_bytes(b.N, b.total_bases, b.flags)));
    int rc = launch_match_stats(ix, stats, a.ms, reinterpret_cast<int32_t *>(a.lohi), stream);
    if (rc) return rc;
    const LuReads R{b.bases, reinterpret_cast<const long long *>(b.read_offsets), (long long)b.N, b.strands()};
    const CtgPair tab = cg ? *cg : CtgPair{{nullptr, 0, 0, 0}, {nullptr, 0, 0, 0}};
    const size_t lds = cg ? ctg_lds_bytes(tab.big) : 0;
    auto count_k = cg ? mem_walk_kernel<false, true> : mem_walk_kernel<false, false>;
    auto fill_k = cg ? mem_walk_kernel<true, true> : mem_walk_kernel<true, false>;
    HIP_TRY(hipMemsetAsync(a.skipped, 0, 8, s));
    if (a.nwin > 0) {
        LAUNCH_SLICED(mem_seed_kernel, mem_seed_kernel, a.nwin, kMemWin, 0, s, ix->dev, R, positions, (int)min_len, (int)max_occ,
                      static_cast<const int32_t *>(a.ms), static_cast<const int2 *>(a.lohi), a.seed, a.pos, a.prev, a.skipped);
        LAUNCH_SLICED(count_k, count_k, a.nwalk, kMemWalk, lds, s, ix->dev, tab, positions, (int)min_len,
                      static_cast<const int32_t *>(a.ms), static_cast<const int2 *>(a.lohi), static_cast<const int2 *>(a.seed),
                      static_cast<const int32_t *>(a.pos), static_cast<const uint8_t *>(a.prev), a.pre, a.kept, a.bsum,
                      static_cast<int4 *>(nullptr), 0ll);
    }
    LAUNCH(scan_block_sums_kernel, dim3(1), dim3(kScanBlock), 0, s, a.bsum, a.nwalk);
    LAUNCH_BLOCKS(mem_offsets_kernel, (b.strand_reads() + 1 + 255) / 256, 256, 0, s, R, positions, a.nwalk,
                  static_cast<const unsigned long long *>(a.kept), static_cast<const unsigned long long *>(a.pre), static_cast<const unsigned long long *>(a.bsum),
                  static_cast<const unsigned long long *>(a.skipped), reinterpret_cast<long long *>(out.offsets),
                  reinterpret_cast<long long *>(out.totals));
    if (out.rows && out.cap_rows > 0 && a.nwin > 0)
        LAUNCH_SLICED(fill_k, fill_k, a.nwalk, kMemWalk, lds, s, ix->dev, tab, positions, (int)min_len,
                      static_cast<const int32_t *>(a.ms), static_cast<const int2 *>(a.lohi), static_cast<const int2 *>(a.seed),
                      static_cast<const int32_t *>(a.pos), static_cast<const uint8_t *>(a.prev), a.pre, a.kept, a.bsum,
                      reinterpret_cast<int4 *>(out.rows), (long long)out.cap_rows);
    return GENIE_OK;
}

int launch_find_mems(const genie_index *ix, const CsrBatch &b, int32_t min_len, int32_t max_occ, const CsrRows &out, void *stream)
{
    return find_mems_any(ix, nullptr, b, min_len, max_occ, out, stream);
}

int64_t find_mems_contigs_workspace_bytes(int64_t N, int64_t total_bases, int32_t flags)
{
    return find_mems_workspace_bytes(N, total_bases, flags);
}

int launch_find_mems_contigs(const genie_index *ix, const ContigTable &ctg, const CsrBatch &b, int32_t min_len, int32_t max_occ,
                             const CsrRows &out, void *stream)
{
    const CtgPair tab{ctg_tab(ctg.offsets, ctg.n_contigs, kCtgWalkSamples), ctg_tab(ctg.offsets, ctg.n_contigs, kCtgSamples)};
    return find_mems_any(ix, &tab, b, min_len, max_occ, out, stream);
}

// contig_stats.inc -- genie_match_stats_contigs and genie_find_smems_contigs: matching statistics and SMEMs that are exact
// with respect to a reference of several sequences (included by kernels.hip behind fwd_step.inc, inside namespace genie).
//
// ms_c[v], the contig-exact matching statistic of a virtual position (long_units.inc), is the largest l for which the l
// bases from there on hold no break and equal T[t .. t+l) for some t with l <= room(t) (contigs.inc): they occur inside ONE
// contig.  Four facts carry the kernels (DESIGN.md section 19 proves them, tests/test_contig_stats_host.py checks them):
//   1  ms_c <= ms, and ms_c >= 1 iff ms >= 1 (an occurrence t < n has room(t) >= 1): absent and bad bases are flagged as ever.
//   2  ms_c[v+1] >= ms_c[v] - 1 inside a strand-read: fwd_c[p] = p + ms_c[p] is non-decreasing, so the traversal of LR3 .. LR5
//      applies to fwd_c unchanged and yields the SMEMs with respect to the sequence set.
//   3  Let p0 be a run start of fwd[] (p0 == 0 or fwd[p0] != fwd[p0-1]).  If some occurrence t of Q[p0 .. fwd[p0]) has
//      room(t) >= fwd[p0] - p0, then ms_c = ms on the whole run (t + k serves p0 + k): only run starts need a room test.
//   4  "some t in the interval of Q[p .. p+l) has room(t) >= l" is monotone in l: where the run start fails, ms_c[p] of every
//      position of the run is found by bisection over l, from the largest room seen upward.
// Both calls are their parents -- lu_run, the parents' tails, lr_match_stats / lr_pipeline -- with the step of long_reads.inc
// set, which puts three kernels between LR2 and what reads fwd[]:
//   LR1, LR2 (MS instance)   fwd[] of the concatenation, nothing else (LUT / RMI mode: the SMEM instance, for its statuses;
//                            its marks are cleared again)
//   CS1 cs_start_kernel      one wave per window, four windows per block, four positions per lane (lr_fwd_kernel's shape;
//                            one block per window, as lr_ms_kernel is cut, took 6.3 ms where this takes the time in
//                            DESIGN.md section 19).  At a run start with a match: its interval as lr_ms_kernel gets it (the
//                            positions the entry does not decide are gathered per wave), then SaRec.s of its rows with early
//                            exit -- one lane up to kCsLaneRows rows, the whole wave beyond (cs_walk: lc_walk_kernel's
//                            shape) -- and room(t) >= len through ctg_find on the staged table.  A run start without a
//                            qualifying row is FLAGGED: the k-th one of a window goes to slot[first position of the window
//                            + k] = {end of the run, position in the window, largest room seen}; the window's count to
//                            wcnt[], the block's to bsum[].
//   scan_block_sums_kernel   over the block counts: item j of the slow list belongs to the last block b with bsum[b] <= j,
//                            and there to the window that wcnt[] says.  No atomic orders anything.
//   CS2 cs_slow_kernel       rare.  A fixed grid of waves strides over the flagged runs (the count stays on the device); a
//                            lane per position of the run searches l (fact 4: l = ms first, a gallop up from the bound, a bisection), l = ms holding where the
//                            position's own interval has a qualifying row; the interval of Q[p .. p+l) is sa_interval's over
//                            the packed unit, its rows are walked by cs_walk.  Writes fwd_c into fwd[] -- only the flagged
//                            run's own positions, whose extent CS1 read before anything was changed -- and counts the
//                            clipped positions, one word per block; cs_totals_kernel adds them to d_totals[0].
//   then, match statistics:  lr_ms_kernel as it is, over the corrected fwd[]: the intervals of clipped positions are those
//                            of the clipped matches in the concatenation.
//   then, SMEMs:             CS3 cs_marks_kernel, one wave per window: what LR2's SMEM instance writes beside fwd[] (the
//                            first maximum of fwd[a] - a, the mark at fwd[a]) from the corrected fwd[]; LR3, LR4,
//                            launch_compact and LR5 as in lr_pipeline.
// What every call with a step shares is in fwd_step.inc: the window's front (fs_window), the intervals of the tested
// positions (fs_intervals), the block totals, cs_totals_kernel, cs_marks_kernel, the sizing (fs_bytes) and the launch
// (fs_match_stats / fs_find_smems).  Here: the area, cs_room, cs_walk, CS1, CS2 and cs_correct, which launches them.
// Workspace: the parent's, then the slots (8 bytes per virtual position), the window and block counts and CS2's clip counts.  The
// parent's part is handed to lu_run at exactly its declared size, so that the units of a pass, and with them the windows,
// never exceed what the counts were sized for (fs_units_cap).
// Memory safety on any table contents is ctg_find's; rows come from the index, positions from fwd[], which LR2 bounds.
namespace {

constexpr int kCsLaneRows = 32;           // an interval of more rows is walked by the whole wave
constexpr int kCsSlowBlocks = 1024;       // blocks of CS2: four flagged runs each per round
constexpr uint32_t kCsRoomCap = 0xFFFFFFu;      // the largest room kept in a slot (a lower bound: capping it is safe)

struct CsArea {
    uint2 *slot;                          // positions: {run end, position in the window << 24 | largest room seen}
    int32_t *wcnt;                        // windows: flagged run starts per window
    unsigned long long *bsum;             // blocks of CS1 + 1: flagged run starts per block, scanned
    unsigned long long *clip;             // kCsSlowBlocks: clipped positions per block of CS2
    long long nwin_cap;                   // windows the counts hold
};

inline int64_t cs_layout(uint8_t *p, int64_t positions, int64_t units, CsArea *a)
{
    a->nwin_cap = positions / kLrWin + units + 1;
    Carver c{p};
    c.take(a->slot, 8 * positions);
    c.take(a->wcnt, 4 * a->nwin_cap);
    c.take(a->bsum, 8 * ((a->nwin_cap + kLrFwdWaves - 1) / kLrFwdWaves + 1));
    c.take(a->clip, 8 * kCsSlowBlocks);
    return c.at;
}

// What the step of a call needs
struct CsCall {
    CtgTab g;
    CsArea a;
    long long *totals;                    // d_totals or null
};

// room of the occurrence at suffix-array row `row`; 0 for the $ suffix
__device__ __forceinline__ int cs_room(const DevIndex &ix, const CtgTab &g, const int *__restrict__ cs, int row)
{
    const int t = ix.sa[row].s;
    return t >= 0 && t < ix.n ? ctg_find(g, cs, ix.n, t).room : 0;
}

// The largest room among the rows [lo, lo + cnt) of a lane's interval, or any room >= len once one is seen (early exit).
// Called by every lane of the wave, cnt == 0 where a lane has nothing to walk.
__device__ __forceinline__ int cs_walk(const DevIndex &ix, const CtgTab &g, const int *__restrict__ cs, int lo, int cnt, int len,
                                       int lane)
{
    int best = 0;
    const bool big = cnt > kCsLaneRows;
    if (!big)
        for (int k = 0; k < cnt; k++) {
            const int room = cs_room(ix, g, cs, lo + k);
            best = room > best ? room : best;
            if (room >= len) break;
        }
    unsigned long long todo = __ballot(big);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int blo = __shfl(lo, src), bcnt = __shfl(cnt, src), blen = __shfl(len, src);
        int top = 0;
        for (int k0 = 0; k0 < bcnt; k0 += kWave) {               // wave-uniform trip count and exit
            const int k = k0 + lane;
            const int room = k < bcnt ? cs_room(ix, g, cs, blo + k) : 0;
            top = room > top ? room : top;
            if (__any(room >= blen)) break;
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const int x = __shfl_xor(top, o);
            top = x > top ? x : top;
        }
        if (lane == src) best = top;
    }
    return best;
}

// CS1.  One wave per window, kLrFwdWaves windows per block (lr_fwd_kernel's shape: four positions per lane, no barrier between
// the staging of the table and the block's count).  The window, skip_flagged and the intervals of the run starts: fwd_step.inc.
template <bool C16, bool SLICED = false>
__global__ void __launch_bounds__(kLrFwdWaves * 64) cs_start_kernel(DevIndex ix, CtgTab cg, int skip_flagged, const long long *__restrict__ off,
                                                                    long long N, long long nwin, const uint64_t *__restrict__ packed,
                                                                    const int32_t *__restrict__ st, const int32_t *__restrict__ fwd,
                                                                    uint2 *__restrict__ slot, int32_t *__restrict__ wcnt,
                                                                    unsigned long long *__restrict__ bsum, long long block0)
{
    constexpr int kPer = kLrWin / kWave;
    extern __shared__ int ctg_lds[];
    __shared__ uint16_t lists[kLrFwdWaves][kLrWin];              // the positions the entry does not decide
    __shared__ int2 sivs[kLrFwdWaves][kLrWin];                   // ... and their intervals
    __shared__ int bcnt[kLrFwdWaves];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const long long blk = SLICED ? block0 + blockIdx.x : (long long)blockIdx.x;
    const long long gw = blk * kLrFwdWaves + wave;
    ctg_stage(cg, ix.n, ctg_lds);
    const FsWin win = fs_window(off, N, gw, st, skip_flagged, gw < nwin);     // wave-uniform; no wave leaves before the barrier
    int nflag = 0;
    if (win.live) {
        const long long o = win.o;
        const int L = win.L, w0 = win.w0;
        const QPlain Q{packed + lr_wd(off, win.r)};
        const unsigned long long below = (1ull << lane) - 1ull;
        int2 iv[kPer];
        int len[kPer], fv[kPer];
        bool start[kPer];
#pragma unroll
        for (int k = 0; k < kPer; k++) {                         // the run starts that have a match
            const int t = k * kWave + lane, a = w0 + t;
            const bool in = t < win.nw;
            fv[k] = in ? fwd[o + a] : 0;
            len[k] = in && (a == 0 || fwd[o + a - 1] != fv[k]) ? fv[k] - a : 0;
            start[k] = len[k] > 0;
        }
        fs_intervals<C16>(ix, Q, fwd, win, lane, start, len, lists[wave], sivs[wave], iv);
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const int t = k * kWave + lane, a = w0 + t;
            const bool act = start[k];
            const int best = cs_walk(ix, cg, ctg_lds, iv[k].x, act ? fs_rows(ix, iv[k]) : 0, len[k], lane);
            const bool flagged = act && best < len[k];
            int p1 = a + 1;
            if (flagged) {                                       // the run's end: the first position behind a whose fwd differs
                int hi = L;
                while (p1 < hi) {
                    const int mid = p1 + ((hi - p1) >> 1);
                    if (fwd[o + mid] == fv[k]) p1 = mid + 1; else hi = mid;
                }
            }
            const unsigned long long fb = __ballot(flagged);
            if (flagged) {
                const uint32_t room = (uint32_t)best < kCsRoomCap ? (uint32_t)best : kCsRoomCap;
                slot[o + w0 + nflag + __popcll(fb & below)] = make_uint2((uint32_t)p1, ((uint32_t)t << 24) | room);
            }
            nflag += __popcll(fb);
        }
    }
    if (lane == 0) {
        if (gw < nwin) wcnt[gw] = nflag;
        bcnt[wave] = nflag;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int all = 0;
        for (int k = 0; k < kLrFwdWaves; k++) all += bcnt[k];
        bsum[blk] = (unsigned long long)all;
    }
}

// CS2.  bsum is scanned: bsum[nblk] flagged runs in all, nblk the blocks of CS1.
__global__ void __launch_bounds__(256) cs_slow_kernel(DevIndex ix, CtgTab cg, const long long *__restrict__ off, long long N,
                                                      long long nwin, const uint64_t *__restrict__ packed, int32_t *__restrict__ fwd,
                                                      const uint2 *__restrict__ slot, const int32_t *__restrict__ wcnt,
                                                      const unsigned long long *__restrict__ bsum, unsigned long long *__restrict__ clip)
{
    extern __shared__ int ctg_lds[];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const long long nblk = (nwin + kLrFwdWaves - 1) / kLrFwdWaves;
    const long long items = (long long)bsum[nblk];
    if ((long long)blockIdx.x * (256 / kWave) >= items) {        // block-uniform: nothing to do, and no staging
        if (threadIdx.x == 0) clip[blockIdx.x] = 0;
        return;
    }
    ctg_stage(cg, ix.n, ctg_lds);
    unsigned long long nclip = 0;
    for (long long j = (long long)blockIdx.x * (256 / kWave) + wave; j < items; j += (long long)gridDim.x * (256 / kWave)) {
        const long long blk = lr_find(nblk, j, [&](long long x) { return (long long)bsum[x]; });
        long long k = j - (long long)bsum[blk], gw = blk * kLrFwdWaves;
        for (int i = 0; i < kLrFwdWaves - 1 && gw + 1 < nwin && k >= wcnt[gw]; i++) k -= wcnt[gw++];      // the window inside its block
        const FsWin win = fs_window(off, N, gw);
        if (!win.live || k < 0 || k >= kLrWin) continue;         // cannot happen: CS1 counted this window
        const long long r = win.r, o = win.o;
        const int L = win.L, w0 = win.w0;
        const uint2 sl = slot[o + w0 + k];
        const int p0 = w0 + (int)(sl.y >> 24), room0 = (int)(sl.y & kCsRoomCap);
        const int p1 = (int)sl.x < L ? (int)sl.x : L;
        if (p0 >= L) continue;
        const int e = fwd[o + p0];                               // the run's fwd: this wave alone writes these positions, below
        const QPlain Q{packed + lr_wd(off, r)};
        for (int c0 = p0; c0 < p1; c0 += kWave) {                // wave-uniform
            const int p = c0 + lane, ms = e - p;
            const bool in = p < p1 && ms > 0;                    // ms == 0: an absent base that ends the run's match
            // pred(lo) holds, pred(hi) does not (ms + 1: no match is that long); the run start failed at ms already
            int lo = 0, hi = 1;
            if (in) {
                lo = room0 - (p - p0) > 1 ? room0 - (p - p0) : 1;
                hi = p == p0 ? ms : ms + 1;
                lo = lo < hi ? lo : hi - 1;
            }
            // The first probe is l = ms; then a gallop upward from lo (1, 2, 4 ... more), where the answer usually sits -- a match
            // cut at its contig's end has ms_c = the room, which is lo --, and a bisection once a length is refuted.
            bool first = p != p0;
            int gal = 1;
            while (__any(hi - lo > 1)) {
                const bool open = hi - lo > 1;
                const bool up = !first && gal > 0;
                const int mid = first ? hi - 1 : (up ? (lo + gal < hi - 1 ? lo + gal : hi - 1) : lo + ((hi - lo) >> 1));
                first = false;
                int2 iv = make_int2(-1, -1);
                if (open) iv = sa_interval(ix, ix.dir, Q, p, mid);
                const int best = cs_walk(ix, cg, ctg_lds, iv.x, open ? fs_rows(ix, iv) : 0, mid, lane);
                if (open) {
                    if (best >= mid) {
                        lo = mid;
                        if (up) gal = gal < (1 << 28) ? gal << 1 : gal;
                    } else {
                        hi = mid;
                        lo = best > lo ? best : lo;              // the rows match mid bases: one with room `best` serves l = best
                        if (up) gal = 0;
                    }
                }
            }
            if (in) {
                nclip += lo < ms ? 1ull : 0ull;
                fwd[o + p] = p + lo;
            }
        }
    }
    const unsigned long long all = fs_block_total(nclip);
    if (threadIdx.x == 0) clip[blockIdx.x] = all;
}

// CS1, the scan, CS2 and the total over the units of `uoff`, whose fwd[] LR2 has written
int cs_correct(const genie_index *ix, const CsCall &cs, bool skip_flagged, const LongArea &a, const long long *uoff, long long U,
               hipStream_t s)
{
    if (a.nwin > cs.a.nwin_cap) return GENIE_E_CAPACITY;         // cannot happen: fs_units_cap
    const size_t lds = ctg_lds_bytes(cs.g);
    const bool c16 = (ix->dev.flags & kFlagCompactTable) != 0;
    const long long nblk = (a.nwin + kLrFwdWaves - 1) / kLrFwdWaves;
    const auto start_one = c16 ? cs_start_kernel<true> : cs_start_kernel<false>;
    const auto start_sliced = c16 ? cs_start_kernel<true, true> : cs_start_kernel<false, true>;
    LAUNCH_SLICED(start_one, start_sliced, nblk, kLrFwdWaves * 64, lds, s, ix->dev, cs.g, (int)skip_flagged, uoff, U, a.nwin,
                  static_cast<const uint64_t *>(a.packed), static_cast<const int32_t *>(a.st), static_cast<const int32_t *>(a.fwd),
                  cs.a.slot, cs.a.wcnt, cs.a.bsum);
    LAUNCH(scan_block_sums_kernel, dim3(1), dim3(kScanBlock), 0, s, cs.a.bsum, nblk);
    const int blocks = (int)std::min<long long>(a.nwin, kCsSlowBlocks);
    LAUNCH(cs_slow_kernel, dim3(blocks), dim3(256), lds, s, ix->dev, cs.g, uoff, U, a.nwin, static_cast<const uint64_t *>(a.packed),
           a.fwd, static_cast<const uint2 *>(cs.a.slot), static_cast<const int32_t *>(cs.a.wcnt),
           static_cast<const unsigned long long *>(cs.a.bsum), cs.a.clip);
    return cs.totals ? fs_totals(cs.a.clip, blocks, cs.totals, s) : GENIE_OK;
}

}  // namespace

int64_t match_stats_contigs_workspace_bytes(int64_t N, int64_t total_bases, int32_t flags)
{
    return fs_bytes(N, total_bases, flags, false, cs_layout);
}

int launch_match_stats_contigs(const genie_index *ix, const ContigTable &ctg, const CsrBatch &b, int32_t *d_ms, int32_t *d_lohi,
                               int64_t *d_totals, void *stream)
{
    CsCall cs{ctg_tab(ctg.offsets, ctg.n_contigs), {}, reinterpret_cast<long long *>(d_totals)};
    return fs_match_stats(ix, 1, b, d_ms, d_lohi, cs, cs_layout, cs_correct, (hipStream_t)stream);
}

int64_t find_smems_contigs_workspace_bytes(int64_t N, int64_t total_bases, int32_t flags)
{
    return fs_bytes(N, total_bases, flags, true, cs_layout);
}

int launch_find_smems_contigs(const genie_index *ix, const ContigTable &ctg, int32_t mode, int32_t min_len, const CsrBatch &b,
                              const CsrRows &out, void *stream)
{
    CsCall cs{ctg_tab(ctg.offsets, ctg.n_contigs), {}, reinterpret_cast<long long *>(out.totals)};
    return fs_find_smems(ix, mode, min_len, 1, b, out, cs, cs_layout, cs_correct, (hipStream_t)stream);
}

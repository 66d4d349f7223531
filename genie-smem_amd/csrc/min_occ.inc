// min_occ.inc -- genie_match_stats_min_occ and genie_find_smems_min_occ: matching statistics and SMEMs under a minimum
// occurrence count k (BWA-MEM's min_intv; included by kernels.hip behind contig_stats.inc, inside namespace genie).
//
// occ(w) is the number of suffix-array rows whose suffix starts with w (the $ row never counts).  ms_k[v], the statistic of
// a virtual position (long_units.inc), is the largest l >= 0 for which the l bases from there on hold no break and occur at
// least k times; fwd_k[p] = p + ms_k[p].  Five facts carry the kernels (DESIGN.md section 21, tests/test_min_occ_host.py):
//   1  ms_k <= ms, ms_k is non-increasing in k, ms_1 = ms.  ms_k[p] = 0 iff the base at p is a break or occurs fewer than k
//      times in the reference: a base RARE AT K ("the reference lacks it" is k = 1).
//   2  ms_k[v+1] >= ms_k[v] - 1 inside a strand-read (dropping the first base can only gain occurrences), so fwd_k is
//      non-decreasing, and "Q[s..e) occurs >= k times" <=> fwd_k[s] >= e (occ is monotone in the length): the traversal of
//      LR3 .. LR5 applied to fwd_k yields exactly the SMEMs under min_intv = k.
//   3  If the interval of Q[p .. fwd[p]) has >= k rows, ms_k = ms from p to the end of p's run of fwd[] (every later match of
//      the run is a suffix of that string).  The run's start serves all of it; so does, for the part of a run that enters a
//      window, the window's first position -- no window looks into another one.
//   4  Otherwise every position is resolved on its own.  occ(Q[p..p+l)) >= k is monotone in l: bisection over [0, ms[p]].
//   5  Without a search over l: let L_j = min(ms, lcp(Q[p..), T[SA[j]..)), which is ms on the interval [lo, hi] of the full
//      match and falls away from it on either side.  Then ms_k[p] is the k-th largest L_j: rows are taken from the two sides
//      of [lo, hi], the larger L first, until k are together (this is max over a of min(ms, lcp(SA[a], SA[a+k-1])) with the
//      window [a, a+k-1] around [lo, hi], evaluated once per row instead of once per window).  0 when fewer than k rows exist.
// Both calls are their parents -- lu_run, the parents' tails, lr_match_stats / lr_pipeline -- with the step of long_reads.inc
// set, as the contig-exact calls are (contig_stats.inc); the front takes k for its mask of usable bases (lu_run).  The step:
//   MO1 mo_resolve_kernel    one wave per window, four windows per block, four positions per lane (cs_start_kernel's shape).
//                            The interval of every run start and of the window's first position, as lr_ms_kernel gets it
//                            (interval_from_window, else sa_interval over the wave's undecided list); a verdict "has k
//                            rows" reaches the positions behind it through two ballots per 64 positions.  The positions of
//                            failed runs are gathered per wave, a lane each: its own interval first (fact 3 from there on
//                            is not used: a lane knows nothing of its neighbours' outcome), then fact 5 for k <= kMoMerge,
//                            fact 4 with sa_interval beyond.  fwd_k goes into fwd[] IN PLACE: a wave reads and writes its own
//                            window alone.  Per window: the positions with ms_k < ms and "some ms_k is 0", one word.
//   MO2 mo_units_kernel      one thread per unit: the sum of its windows' counts, and GENIE_READ_ABSENT_BASE for a unit that
//                            holds a base rare at k (so no kernel reads a status that another block of it is writing).  The
//                            counts of the units that keep their rows (SMEMs) or have statistics at all (not a bad base),
//                            one word per block; cs_totals_kernel adds them to d_totals[0].  A position counts when ms_k is
//                            shorter than fwd[] of ITS UNIT says: with SPLIT_BREAKS a rare base is a break for both.
//   then lr_ms_kernel as it is, or cs_marks_kernel and LR3 .. LR5, over the corrected fwd[].
// The window's front, the intervals of the tested positions, the block totals, cs_totals_kernel, cs_marks_kernel, the sizing
// and the launch are the ones every call with a step uses: fwd_step.inc.
// Workspace: the parent's at exactly its declared size (fs_units_cap), then the window words and MO2's block counts.
// Memory safety: rows are clamped to [1, n], reference positions to [0, n); positions come from fwd[], which LR2 bounds.
namespace {

constexpr int kMoMerge = 32;              // k up to here: fact 5, beyond: fact 4
constexpr int32_t kMoRare = 1 << 16;      // in a window's word: some position of it has ms_k == 0 < ms

struct MoArea {
    int32_t *wcnt;                        // windows: clipped positions | kMoRare
    unsigned long long *clip;             // blocks of MO2: clipped positions of the units that count
    long long nwin_cap, unit_cap;
};

inline int64_t mo_layout(uint8_t *p, int64_t positions, int64_t units, MoArea *a)
{
    a->nwin_cap = positions / kLrWin + units + 1;
    a->unit_cap = units;
    Carver c{p};
    c.take(a->wcnt, 4 * a->nwin_cap);
    c.take(a->clip, 8 * ((units + 255) / 256 + 1));
    return c.at;
}

struct MoCall {
    int32_t k;
    MoArea a;
    long long *totals;                    // d_totals or null
};

// min(cap, lcp(T[s0..), T[SA[row]..))); w0 = rwin(ref, s0).  row in [1, n].
__device__ __forceinline__ int mo_lcp(const DevIndex &ix, int s0, uint64_t w0, int row, int cap)
{
    const int t = ix.sa[row].s;
    if (t < 0 || t >= ix.n) return 0;
    const int far = ix.n - (t > s0 ? t : s0);
    const int lim = far < cap ? far : cap;
    int l = 0;
    while (l < lim) {
        const uint64_t x = rwin(ix.ref, t + l) ^ (l ? rwin(ix.ref, s0 + l) : w0);
        if (x) { l += __clzll((long long)x) >> 1; break; }
        l += 32;
    }
    return l < lim ? l : lim;
}

// ms_k of the position a of Q whose full match of ms > 0 bases has the interval iv of fewer than k rows
template <class Q>
__device__ __forceinline__ int mo_resolve(const DevIndex &ix, const Q qp, int a, int ms, int2 iv, int k)
{
    const int c = fs_rows(ix, iv);
    if (k <= kMoMerge && c > 0) {                                // fact 5: the k-th largest L_j
        const int s0 = ix.sa[iv.x].s;
        if (s0 < 0 || s0 >= ix.n) return 0;
        const uint64_t w0 = rwin(ix.ref, s0);
        int left = iv.x - 1, right = iv.x + c;
        int ll = left >= 1 ? mo_lcp(ix, s0, w0, left, ms) : -1;  // -1: no row on that side
        int lr = right <= ix.n ? mo_lcp(ix, s0, w0, right, ms) : -1;
        int l = ms;
        for (int need = k - c; need > 0 && l > 0; need--) {
            if (ll < 0 && lr < 0) return 0;
            if (ll >= lr) {
                l = ll;
                left--;
                ll = left >= 1 ? mo_lcp(ix, s0, w0, left, l) : -1;       // no later row counts for more than l
            } else {
                l = lr;
                right++;
                lr = right <= ix.n ? mo_lcp(ix, s0, w0, right, l) : -1;
            }
        }
        return l;
    }
    int lo = 0, hi = ms;                                         // fact 4: hi fails, lo holds or is the floor
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (fs_rows(ix, sa_interval(ix, ix.dir, qp, a, mid)) >= k) lo = mid; else hi = mid;
    }
    return lo;
}

// MO1.  The window, skip_flagged and the intervals of the tested positions: fwd_step.inc.
template <bool C16, bool SLICED = false>
__global__ void __launch_bounds__(kLrFwdWaves * 64) mo_resolve_kernel(DevIndex ix, int kocc, int skip_flagged, const long long *__restrict__ off,
                                                                      long long N, long long nwin, const uint64_t *__restrict__ packed,
                                                                      const int32_t *__restrict__ st, int32_t *fwd,
                                                                      int32_t *__restrict__ wcnt, long long block0)
{
    constexpr int kPer = kLrWin / kWave;
    __shared__ uint16_t lists[kLrFwdWaves][kLrWin];              // the positions the entry does not decide; then those to resolve
    __shared__ int2 sivs[kLrFwdWaves][kLrWin];                   // their intervals
    __shared__ int32_t slen[kLrFwdWaves][kLrWin];                // ms of the positions to resolve
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const long long blk = SLICED ? block0 + blockIdx.x : (long long)blockIdx.x;
    const long long gw = blk * kLrFwdWaves + wave;
    if (gw >= nwin) return;                                      // wave-uniform; no block-wide barrier below
    const FsWin win = fs_window(off, N, gw, st, skip_flagged);
    int nclip = 0;
    bool rare = false;
    if (win.live) {
        const long long o = win.o;
        const int w0 = win.w0;
        const QPlain Q{packed + lr_wd(off, win.r)};
        uint16_t *sl = lists[wave];
        int2 *sv = sivs[wave];
        int32_t *sn = slen[wave];
        const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
        int2 iv[kPer];
        int len[kPer];
        bool tested[kPer];
#pragma unroll
        for (int k = 0; k < kPer; k++) {                         // the run starts and the window's first position
            const int t = k * kWave + lane, a = w0 + t;
            const bool in = t < win.nw;
            const int fv = in ? fwd[o + a] : 0;
            len[k] = in ? fv - a : 0;
            tested[k] = len[k] > 0 && (t == 0 || fwd[o + a - 1] != fv);
        }
        fs_intervals<C16>(ix, Q, fwd, win, lane, tested, len, sl, sv, iv);
        wave_lds_fence();                                        // the list and the intervals are taken: both are reused
        // the verdict of the last tested position at or in front of every position (fact 3), then the list of the others
        bool carry = true;                                       // wave-uniform: the verdict that enters the next 64 positions
        int nres = 0;
#pragma unroll
        for (int k = 0; k < kPer; k++) {
            const int t = k * kWave + lane;
            const bool pass = tested[k] && fs_rows(ix, iv[k]) >= kocc;
            const unsigned long long tb = __ballot(tested[k]), pb = __ballot(pass);
            const unsigned long long mine = tb & upto;
            const bool ok = mine ? ((pb >> (63 - __clzll((long long)mine))) & 1ull) != 0 : carry;
            if (tb) carry = ((pb >> (63 - __clzll((long long)tb))) & 1ull) != 0;
            const bool res = len[k] > 0 && !ok;
            const unsigned long long rb = __ballot(res);
            if (res) {
                sl[nres + __popcll(rb & below)] = (uint16_t)t;
                sv[t] = tested[k] ? iv[k] : make_int2(0, -2);    // (0, -2): not taken yet
                sn[t] = len[k];
            }
            nres += __popcll(rb);
        }
        wave_lds_fence();
        for (int c0 = 0; c0 < nres; c0 += kWave) {               // a lane per position of a failed run
            const bool have = c0 + lane < nres;
            const int t = have ? sl[c0 + lane] : 0, a = w0 + t, ms = have ? sn[t] : 0;
            int2 v = have ? sv[t] : make_int2(-1, -1);
            const bool take = have && v.y == -2;                 // its own interval, as above
            int2 e;
            const bool fast = interval_from_window<C16>(ix, take ? Q.win(a) : 0ull, ms, take, e);
            if (take) v = fast ? e : sa_interval(ix, ix.dir, Q, a, ms);
            if (have && fs_rows(ix, v) < kocc) {
                const int l = mo_resolve(ix, Q, a, ms, v, kocc);
                if (l < ms) {
                    fwd[o + a] = a + l;
                    nclip++;
                    rare = rare || l == 0;
                }
            }
        }
    }
    nclip = (int)wave_sum64((unsigned long long)nclip);
    const bool any_rare = __any(rare);
    if (lane == 0) wcnt[gw] = nclip | (any_rare ? kMoRare : 0);
}

// MO2.  One thread per unit.
__global__ void __launch_bounds__(256) mo_units_kernel(const long long *__restrict__ off, long long N, int skip_flagged,
                                                       int32_t *__restrict__ st, const int32_t *__restrict__ wcnt,
                                                       unsigned long long *__restrict__ clip)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long d = 0;
    if (r < N) {
        const long long Ll = off[r + 1] - off[r], wb = lr_wb(off, r);
        const long long nw = (Ll + kLrWin - 1) / kLrWin;
        int32_t status = st[r];
        bool rare = false;
        for (long long i = 0; i < nw; i++) {
            const int32_t c = wcnt[wb + i];
            d += (unsigned long long)(c & (kMoRare - 1));
            rare = rare || (c & kMoRare) != 0;
        }
        if (rare && status == GENIE_READ_OK) st[r] = status = GENIE_READ_ABSENT_BASE;
        if (skip_flagged ? status != GENIE_READ_OK : status == GENIE_READ_BAD_BASE) d = 0;
    }
    const unsigned long long all = fs_block_total(d);
    if (threadIdx.x == 0) clip[blockIdx.x] = all;
}

// MO1, MO2 and the total over the units of `uoff`, whose fwd[] LR2 has written
int mo_correct(const genie_index *ix, const MoCall &mo, bool skip_flagged, const LongArea &a, const long long *uoff, long long U,
               hipStream_t s)
{
    if (a.nwin > mo.a.nwin_cap || U > mo.a.unit_cap) return GENIE_E_CAPACITY;     // cannot happen: fs_units_cap
    const bool c16 = (ix->dev.flags & kFlagCompactTable) != 0;
    const long long nblk = (a.nwin + kLrFwdWaves - 1) / kLrFwdWaves;
    const auto one = c16 ? mo_resolve_kernel<true> : mo_resolve_kernel<false>;
    const auto sliced = c16 ? mo_resolve_kernel<true, true> : mo_resolve_kernel<false, true>;
    LAUNCH_SLICED(one, sliced, nblk, kLrFwdWaves * 64, 0, s, ix->dev, (int)mo.k, (int)skip_flagged, uoff, U, a.nwin,
                  static_cast<const uint64_t *>(a.packed), static_cast<const int32_t *>(a.st), a.fwd, mo.a.wcnt);
    const long long ublk = (U + 255) / 256;
    LAUNCH_BLOCKS(mo_units_kernel, ublk, 256, 0, s, uoff, U, (int)skip_flagged, a.st, static_cast<const int32_t *>(mo.a.wcnt), mo.a.clip);
    return mo.totals ? fs_totals(mo.a.clip, (int)ublk, mo.totals, s) : GENIE_OK;
}

}  // namespace

int64_t match_stats_min_occ_workspace_bytes(int64_t N, int64_t total_bases, int32_t flags)
{
    return fs_bytes(N, total_bases, flags, false, mo_layout);
}

// The front cuts at the bases rare at k
int launch_match_stats_min_occ(const genie_index *ix, int32_t min_occ, const CsrBatch &b, int32_t *d_ms, int32_t *d_lohi,
                               int64_t *d_totals, void *stream)
{
    MoCall mo{min_occ, {}, reinterpret_cast<long long *>(d_totals)};
    return fs_match_stats(ix, min_occ, b, d_ms, d_lohi, mo, mo_layout, mo_correct, (hipStream_t)stream);
}

int64_t find_smems_min_occ_workspace_bytes(int64_t N, int64_t total_bases, int32_t flags)
{
    return fs_bytes(N, total_bases, flags, true, mo_layout);
}

int launch_find_smems_min_occ(const genie_index *ix, int32_t mode, int32_t min_len, int32_t min_occ, const CsrBatch &b,
                              const CsrRows &out, void *stream)
{
    MoCall mo{min_occ, {}, reinterpret_cast<long long *>(out.totals)};
    return fs_find_smems(ix, mode, min_len, min_occ, b, out, mo, mo_layout, mo_correct, (hipStream_t)stream);
}

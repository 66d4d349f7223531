// fwd_step.inc -- what the calls with a step share (included by kernels.hip behind contigs.inc, inside namespace genie).
//
// A step is the LrStep hook of long_reads.inc: it rewrites fwd[] in place between LR2 and whatever reads fwd[].  A call
// with a step is its parent -- lu_run, the parent's tail, lr_match_stats / lr_pipeline -- on the parent's part of the
// workspace at exactly its declared size, with the step's own area behind it.  The contig-exact calls (contig_stats.inc)
// and the min_occ calls (min_occ.inc) are such calls; each of them names its area's layout and its corrector, the rest is
// here:
//   host     fs_units_cap, fs_bytes ("the parent's bytes plus the step's area"), fs_launch with its two bindings
//            fs_match_stats and fs_find_smems, the launchers fs_totals and fs_marks
//   device   fs_window (a window's read, extent and status rule), fs_intervals (the suffix-array intervals of chosen
//            positions of a window), fs_block_total, fs_rows
//   kernels  cs_totals_kernel, cs_marks_kernel (CS3): both families launch them; they keep the names the profiles know
namespace {

// rows of an inclusive interval that are followed: none for (-1, -1), none beyond the suffix array
__device__ __forceinline__ int fs_rows(const DevIndex &ix, int2 iv)
{
    const int hi = iv.y < ix.n ? iv.y : ix.n;
    return iv.x >= 0 && hi >= iv.x ? hi - iv.x + 1 : 0;
}

// Window gw of the units of `off`: positions [w0, w0 + nw) of unit r, whose L bases start at o.  live: the window lies inside
// its unit (there is at most one window past a unit's end) and, given st, the unit's status admits it.  skip_flagged: the
// SMEM tail, where a unit with any status has no rows (and, in LUT / RMI mode, no fwd[]); the match statistics want every
// unit but those with a bad base.  some: false for a wave that has no window of the batch (gw >= nwin) and may not return,
// because a block barrier follows.  Wave-uniform where gw is.
struct FsWin {
    long long r, o;
    int L, w0, nw;
    bool live;
};

__device__ __forceinline__ FsWin fs_window(const long long *__restrict__ off, long long N, long long gw, bool some = true)
{
    FsWin v{0, 0, 0, 0, 0, some};
    if (v.live) {
        v.r = lr_find(N, gw, [&](long long x) { return lr_wb(off, x); });
        const long long w = gw - lr_wb(off, v.r);
        v.o = off[v.r];
        const long long Ll = off[v.r + 1] - v.o;
        v.live = w >= 0 && w * kLrWin < Ll;
        v.L = (int)Ll;
        v.w0 = (int)(w * kLrWin);
        v.nw = v.L - v.w0 < kLrWin ? v.L - v.w0 : kLrWin;
    }
    return v;
}

__device__ __forceinline__ FsWin fs_window(const long long *__restrict__ off, long long N, long long gw, const int32_t *__restrict__ st,
                                           int skip_flagged, bool some = true)
{
    FsWin v = fs_window(off, N, gw, some);
    if (v.live) {
        const int32_t status = st[v.r];
        v.live = skip_flagged ? status == GENIE_READ_OK : status != GENIE_READ_BAD_BASE;
    }
    return v;
}

// The intervals of the tested positions of window v, as lr_ms_kernel gets them: position t = k * kWave + lane of the window
// is tested[k] and its match has len[k] bases (what fwd[] says; > 0 where tested).  interval_from_window decides most; the
// others are gathered into the wave's list sl[kLrWin] by ballot and searched by sa_interval on full waves, through the
// wave's rows sv[kLrWin]; a lane knows its listed positions by iv[k].y in the meantime, which costs no register.  iv[k] of
// an untested position is what interval_from_window leaves there.  Called by the whole wave; sl and sv are free again behind
// a wave_lds_fence.
template <bool C16>
__device__ __forceinline__ void fs_intervals(const DevIndex &ix, const QPlain &Q, const int32_t *fwd, const FsWin &v, int lane,
                                             const bool (&tested)[kLrWin / kWave], const int (&len)[kLrWin / kWave], uint16_t *sl,
                                             int2 *sv, int2 (&iv)[kLrWin / kWave])
{
    constexpr int kPer = kLrWin / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;
    constexpr int kListed = INT32_MIN;                           // iv[k].y of a position on the list: no interval ends there
    int ngen = 0;
#pragma unroll
    for (int k = 0; k < kPer; k++) {
        const int t = k * kWave + lane;
        const uint64_t x = tested[k] ? Q.win(v.w0 + t) : 0ull;
        const bool fast = interval_from_window<C16>(ix, x, len[k], tested[k], iv[k]);
        const bool general = tested[k] && !fast;
        const unsigned long long gb = __ballot(general);
        if (general) {
            sl[ngen + __popcll(gb & below)] = (uint16_t)t;
            iv[k].y = kListed;
        }
        ngen += __popcll(gb);
    }
    wave_lds_fence();
    for (int c0 = 0; c0 < ngen; c0 += kWave) {                   // the general search on full waves
        if (c0 + lane < ngen) {
            const int g = sl[c0 + lane], ga = v.w0 + g;
            sv[g] = sa_interval(ix, ix.dir, Q, ga, fwd[v.o + ga] - ga);
        }
    }
    wave_lds_fence();
#pragma unroll
    for (int k = 0; k < kPer; k++)
        if (iv[k].y == kListed) iv[k] = sv[k * kWave + lane];
}

// The sum of v over a block of 256 threads; thread 0 has it.  One barrier: every thread of the block calls.
__device__ __forceinline__ unsigned long long fs_block_total(unsigned long long v)
{
    __shared__ unsigned long long wsum[256 / kWave];
    v = wave_sum64(v);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = v;
    __syncthreads();
    unsigned long long all = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < 256 / kWave; k++) all += wsum[k];
    return all;
}

// d_totals[0] += the blocks' counts (one block; the passes of a call follow each other on the stream)
__global__ void __launch_bounds__(256) cs_totals_kernel(const unsigned long long *__restrict__ clip, int blocks,
                                                        long long *__restrict__ totals)
{
    unsigned long long d = 0;
    for (int b = threadIdx.x; b < blocks; b += 256) d += clip[b];
    const unsigned long long all = fs_block_total(d);
    if (threadIdx.x == 0) totals[0] += (long long)all;
}

int fs_totals(const unsigned long long *clip, int blocks, long long *totals, hipStream_t s)
{
    LAUNCH(cs_totals_kernel, dim3(1), dim3(256), 0, s, clip, blocks, totals);
    return GENIE_OK;
}

// CS3: the window maxima and the marks of LR2's SMEM instance, from fwd[] as it stands
template <bool SLICED>
__global__ void __launch_bounds__(kLrFwdWaves * 64) cs_marks_kernel(const long long *__restrict__ off, long long N, long long nwin,
                                                                    const int32_t *__restrict__ st, const int32_t *__restrict__ fwd,
                                                                    int2 *__restrict__ wmax, uint8_t *__restrict__ mark,
                                                                    long long block0)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const long long gw = (SLICED ? block0 + blockIdx.x : (long long)blockIdx.x) * kLrFwdWaves + wave;
    if (gw >= nwin) return;                                      // wave-uniform; no block-wide barrier below
    const FsWin v = fs_window(off, N, gw, st, 1);
    if (!v.live) return;
    unsigned long long best = 0;                                 // (fwd[a] - a) << 8 | 255 - (a - w0): the first maximum
#pragma unroll
    for (int k = 0; k < kLrWin / kWave; k++) {
        const int t = k * kWave + lane, a = v.w0 + t;
        if (t < v.nw) {
            const int e = fwd[v.o + a];
            const unsigned long long key = ((unsigned long long)(uint32_t)(e - a) << kLrWinShift) | (unsigned)(kLrWin - 1 - t);
            best = key > best ? key : best;
            if (e >= 0 && e < v.L) mark[v.o + e] = 1;            // every writer stores the same value
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned long long x = lr_shfl_xor64(best, m);
        best = x > best ? x : best;
    }
    if (lane == 0) wmax[gw] = make_int2((int)(best >> kLrWinShift), v.w0 + kLrWin - 1 - (int)(best & (kLrWin - 1)));
}

// CS3 over the units of `uoff`: LR3 finds in a.wmax and a.mark what LR2's SMEM instance would have left there
int fs_marks(const LongArea &a, const long long *uoff, long long U, hipStream_t s)
{
    LAUNCH_SLICED(cs_marks_kernel<false>, cs_marks_kernel<true>, (a.nwin + kLrFwdWaves - 1) / kLrFwdWaves, kLrFwdWaves * 64, 0, s, uoff, U,
                  a.nwin, static_cast<const int32_t *>(a.st), static_cast<const int32_t *>(a.fwd), a.wmax, a.mark);
    return GENIE_OK;
}

// The most units a pass of lu_run takes when the parent's part of the workspace has exactly its declared size: the
// strand-reads without SPLIT_BREAKS, else what long_ex_pass_units, which lu_run asks too, finds for any number of units
// (the padding of the pieces can admit a few more than long_ex_units).  A step's area is sized for them: the units of a
// pass, and with them the windows, never exceed it.
inline int64_t fs_units_cap(int64_t N, int64_t total, int32_t flags, bool smems)
{
    const int S = (flags & GENIE_READS_BOTH_STRANDS) ? 2 : 1;
    const bool split = (flags & GENIE_READS_SPLIT_BREAKS) != 0;
    const int64_t SN = std::max<int64_t>(1, (int64_t)S * N);
    if (!split) return SN;
    LongExFixed f;
    const int64_t avail = long_ex_bytes(N, total, flags, smems) - long_ex_fixed_layout(nullptr, N, total, S, split, &f);
    return long_ex_pass_units(SN, SN + (int64_t)S * total + 1, total, S, avail, smems, true);
}

// The workspace of a call with a step: the parent's bytes plus the step's area, layout(p, virtual positions, units, area).
// With a base the area is carved behind the parent's part.
template <class Area>
inline int64_t fs_bytes(int64_t N, int64_t total, int32_t flags, bool smems, int64_t (*layout)(uint8_t *, int64_t, int64_t, Area *),
                        uint8_t *base = nullptr, Area *a = nullptr)
{
    Area sized;
    const int S = (flags & GENIE_READS_BOTH_STRANDS) ? 2 : 1;
    const int64_t parent = long_ex_bytes(N, total, flags, smems);
    return parent + layout(base ? base + parent : nullptr, (int64_t)S * total, fs_units_cap(N, total, flags, smems), a ? a : &sized);
}

// A call with a step.  call: what the step needs, with its area `a` (carved here) and `totals` (d_totals or null, zeroed
// here); correct(ix, call, skip_flagged, area of the pass, uoff, U, stream) is the step, behind which the SMEM tail wants
// CS3.  make_tail(parent batch, step) gives the parent's tail.
template <class Call, class Layout, class Correct, class MakeTail>
int fs_launch(const genie_index *ix, int32_t mode, int32_t min_occ, const CsrBatch &b, Call &call, Layout layout, Correct correct,
              hipStream_t s, MakeTail make_tail)
{
    using Tail = decltype(make_tail(b, LrStep{}));
    constexpr bool smems = Tail::kSmems;
    if (call.totals) HIP_TRY(hipMemsetAsync(call.totals, 0, 8, s));
    if (b.N > 0) fs_bytes(b.N, b.total_bases, b.flags, smems, layout, static_cast<uint8_t *>(b.ws), &call.a);
    CsrBatch parent = b;
    parent.ws_bytes = long_ex_bytes(b.N, b.total_bases, b.flags, smems);
    Tail tail = make_tail(parent, [&](const LongArea &a, const long long *uoff, long long U) {
        const int rc = correct(ix, call, smems, a, uoff, U, s);
        return rc || !smems ? rc : fs_marks(a, uoff, U, s);
    });
    return lu_run(ix, mode, parent, s, tail, min_occ);
}

// genie_match_stats with a step; min_occ: the front's mask of usable bases (lu_run), 1 for all that occur
template <class Call, class Layout, class Correct>
int fs_match_stats(const genie_index *ix, int32_t min_occ, const CsrBatch &b, int32_t *d_ms, int32_t *d_lohi, Call &call,
                   Layout layout, Correct correct, hipStream_t s)
{
    return fs_launch(ix, GENIE_MODE_BWA, min_occ, b, call, layout, correct, s,
                     [&](const CsrBatch &parent, LrStep step) { return LuMsTail{ix, parent, d_ms, d_lohi, s, std::move(step)}; });
}

// genie_find_smems_long_ex with a step
template <class Call, class Layout, class Correct>
int fs_find_smems(const genie_index *ix, int32_t mode, int32_t min_len, int32_t min_occ, const CsrBatch &b, const CsrRows &out,
                  Call &call, Layout layout, Correct correct, hipStream_t s)
{
    return fs_launch(ix, mode, min_occ, b, call, layout, correct, s, [&](const CsrBatch &parent, LrStep step) {
        return LuSmemTail{ix, mode, min_len, parent, out, s, std::move(step)};
    });
}

}  // namespace

// long_reads.inc -- the SMEM pipeline for reads of any length, over UNITS given as CSR (included by kernels.hip, inside
// namespace genie; uses its launch plumbing and the match-statistics helpers of match_table_kernel.inc).  A unit is a run
// of bases that is searched as one read: uoff[U + 1] are the units' offsets (prefix sums of their lengths), usrc[u] says
// where unit u's bases come from, ushift[u] where it starts inside its read.  Without usrc unit u is the caller's bytes
// [uoff[u], uoff[u + 1]) read forwards, without ushift it starts at 0: genie_find_smems_long's reads are such units.
// long_units.inc makes the units and holds the entry point.
//
// The fixed-stride pipeline keeps a whole read in LDS and its positions in 16 bits.  Here nothing is per unit except one
// short serial pass: every stage is cut into WINDOWS of kLrWin positions (unit-relative: window w of a unit holds its
// positions [w kLrWin, (w + 1) kLrWin)), handed out across all units of the batch, so ten 10^6-base reads fill the chip
// as well as 10^6 short ones.  Positions are 32-bit.  lr_pipeline launches, over (uoff, U):
//   LR1 lr_pack_kernel    one thread per 64-bit word of the packed stream (32 bases, plain big-endian words as QPlain
//                         reads them); unit u owns the words [Wd(u), Wd(u+1)), Wd(u) = uoff[u] / 32 + 3u, which leaves at
//                         least two zero words behind every unit (the padding every 32-base window relies on).  Only this
//                         stage reads the caller's bases: a reversed unit is read backwards and complemented after the
//                         bad-base test on the raw bytes (the reverse complement is never written as bytes).  Bad base:
//                         the unit's status.
//   LR2 lr_fwd_kernel     one wave per window: matching statistics fwd[a] (end of the longest match at a, 32-bit) from
//                         one match-table lookup per position (mt_issue / mt_eval, as round 1 of K_A); positions the entry
//                         cannot decide go to the slow list (mt_slow, the same code as K_A's), which compares the read with
//                         the reference for as long as they agree -- past the window, to the end of the unit.  Also:
//                         the window's maximum of fwd[a] - a (first position on ties), the mark "some position's match
//                         ends here" at fwd[a], and the absent-base flag (fwd[a] = a).
//   LR3 lr_walk_kernel    one block per window, its fwd and the previous window's in LDS.  The traversal step of K_B depends only on the current end i: the
//                         candidates are the positions b <= i with fwd[b] > i, a range [lo(i), i] (fwd[] is
//                         non-decreasing), the winner b* the first maximum of fwd[b] - b, the next end fwd[b*].  Only
//                         0 and the values of fwd[] can be ends, so only marked positions take the step: a scan down from i
//                         that takes whole windows from their maxima (LR2) where fwd at the window's first position still
//                         covers i.  Then pointer jumping in LDS (log2 kLrWin rounds) gives, for every marked position e,
//                         the first end at or behind the window's end reached from e and the rows emitted on the way.
//   LR4 lr_chain_kernel   one thread per unit: the chain from 0, one step per window it enters (not per SMEM).  Writes the
//                         window's entry end and the rows emitted before it in the unit; the unit's row count.
//   launch_compact        the unit counts to `offsets` (offsets only).
//   LR5 lr_emit_kernel    one thread per window the chain enters: its SMEMs in order, the SA interval of each from
//                         sa_interval over the packed unit (any length), each row written once, non-temporal, with the
//                         unit's start inside its read added to start / end.
// lr_match_stats launches LR1 and LR2 alone (lr_fwd_kernel<C16, true>: no maxima, no marks, and a window goes on where
// another one has flagged its unit's absent base), then
//   LRM lr_ms_kernel      one block per window, one lane per position: fwd[a] - a to the position's place in the caller's
//                         array, and the SA interval of [a, fwd[a]) from the match-table entry of the position's P2-mer where
//                         that decides (interval_from_window, as K_C), else from sa_interval over the packed unit -- those
//                         positions are gathered per block so that the search runs on full waves.
// Both sequences take an optional step (LrStep) that runs behind LR2 and corrects fwd[] before anything reads it: the
// contig-exact calls (contig_stats.inc) are their parents with that step set.
namespace {

constexpr int kLrWin = 256;               // positions per window (a multiple of 64: one per lane of LR3's block)
constexpr int kLrWinShift = 8;
constexpr int kLrFwdWaves = 4;            // windows per LR2 block
static_assert((1 << kLrWinShift) == kLrWin, "window shift");

__device__ __forceinline__ long long lr_wd(const long long *off, long long r) { return off[r] / 32 + 3 * r; }          // first packed word
__device__ __forceinline__ long long lr_wb(const long long *off, long long r) { return off[r] / kLrWin + r; }      // first window

// The read r in [0, N) with key(r) <= g < key(r + 1) (key non-decreasing; r = 0 when g < key(0)).
template <class F>
__device__ __forceinline__ long long lr_find(long long N, long long g, F key)
{
    long long lo = 0, hi = N - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (key(mid) <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ unsigned long long lr_shfl_xor64(unsigned long long v, int m)
{
    const unsigned int lo = (unsigned)__shfl_xor((int)(unsigned)v, m, kWave);
    const unsigned int hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, kWave);
    return ((unsigned long long)hi << 32) | lo;
}

// usrc[u]: (source byte of unit u's first base) * 2 + reversed; null: every unit is forward and starts at byte uoff[u]
__global__ void __launch_bounds__(256) lr_pack_kernel(const uint8_t *__restrict__ bases, const long long *__restrict__ uoff, long long U,
                                                      const long long *__restrict__ usrc, long long nwords,
                                                      uint64_t *__restrict__ packed, int32_t *__restrict__ st)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nwords) return;
    const long long u = lr_find(U, g, [&](long long x) { return lr_wd(uoff, x); });
    const long long k = g - lr_wd(uoff, u);
    const long long L = uoff[u + 1] - uoff[u];
    uint64_t w = 0;
    if (k >= 0 && 32 * k < L) {
        const long long key = usrc ? usrc[u] : 2 * uoff[u];
        const int cnt = L - 32 * k < 32 ? (int)(L - 32 * k) : 32;
        uint32_t bad = 0;
        if (key & 1) {                                           // reversed: base j of the word is source byte -j, complemented
            const uint8_t *src = bases + (key >> 1) - 32 * k;
            for (int j = 0; j < cnt; j++) {
                const uint32_t c = src[-j];
                bad |= c;
                w |= (uint64_t)((c & 3u) ^ 3u) << (62 - 2 * j);
            }
        } else {
            const uint8_t *src = bases + (key >> 1) + 32 * k;
            for (int j = 0; j < cnt; j++) {
                const uint32_t c = src[j];
                bad |= c;
                w |= (uint64_t)(c & 3u) << (62 - 2 * j);
            }
        }
        if (bad > 3u) st[u] = GENIE_READ_BAD_BASE;            // every writer stores the same value
    }
    packed[g] = w;
}

// LR2, LR3 and LRM take the first block (LR2) or window (LR3, LRM) of their launch as their last argument: a batch of 2^24
// windows or more is launched in slices through the SLICED instance (LAUNCH_SLICED); any other batch is one launch of the
// instance that does not read it, the kernel as it was.
// MS (the match-statistics tail): fwd[] alone -- wmax and mark are not touched -- and only a bad base stops a window: fwd[]
// of a unit with an absent base is still wanted, and another window of the unit may have flagged it already.
template <bool C16, bool MS = false, bool SLICED = false>
__global__ void __launch_bounds__(kLrFwdWaves * 64) lr_fwd_kernel(DevIndex ix, int mode, const long long *__restrict__ off, long long N,
                                                                  long long nwin, const uint64_t *__restrict__ packed,
                                                                  int32_t *__restrict__ st, int32_t *__restrict__ fwd,
                                                                  int2 *__restrict__ wmax, uint8_t *__restrict__ mark,
                                                                  long long mtab_bytes, long long block0)
{
    __shared__ uint16_t lists[kLrFwdWaves][kLrWin];
    __shared__ int32_t rows[kLrFwdWaves][kLrWin];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const long long gw = (SLICED ? block0 + blockIdx.x : (long long)blockIdx.x) * kLrFwdWaves + wave;
    if (gw >= nwin) return;                                      // wave-uniform; no block-wide barrier below
    const long long r = lr_find(N, gw, [&](long long x) { return lr_wb(off, x); });
    const long long w = gw - lr_wb(off, r);
    const long long o = off[r], Ll = off[r + 1] - o;
    if (w < 0 || w * kLrWin >= Ll) return;                     // a window past the read's end (at most one per read)
    const int L = (int)Ll, w0 = (int)(w * kLrWin);
    if (MS ? st[r] == GENIE_READ_BAD_BASE : st[r] != GENIE_READ_OK) return;      // bad base or too short (LR0 / LR1)
    const __amdgpu_buffer_rsrc_t mtab =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<MatchRec *>(ix.mtab), 0, (int)mtab_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ov =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<MatchOv16 *>(ix.ov), 0, ix.ov_entries * (int)sizeof(MatchOv16), 0x00020000);
    const uint64_t *q = packed + lr_wd(off, r);
    const QPlain Q{q};
    uint16_t *sl = lists[wave];
    int32_t *fw = rows[wave];
    const int nw = L - w0 < kLrWin ? L - w0 : kLrWin;
    int nslow = 0;
#pragma unroll
    for (int k = 0; k < kLrWin / kWave; k++) {
        const int t = k * kWave + lane, a = w0 + t;
        bool slow = false;
        if (t < nw) {
            const uint64_t x = Q.win(a);
            const MtProbe p = mt_issue<C16>(mtab, (uint32_t)(x >> 32), (uint32_t)x, ix.P2);
            const mt_v4i rb = mt_second<C16>(mtab, p);
            bool s;
            const int b0 = mt_eval<C16>(p, rb, ix.P2, s);
            const int m = L - a;
            slow = s && m > b0;
            fw[t] = a + (b0 < m ? b0 : m);
        }
        const uint64_t bal = __ballot(slow);
        if (slow) sl[nslow + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)t;
        nslow += __popcll(bal);
    }
    wave_lds_fence();
    for (int c0 = 0; c0 < nslow; c0 += kWave)
        mt_slow<true, C16, QPlain, int32_t>(ix, mtab, ov, mode, lane, c0, nslow, sl, reinterpret_cast<const uint32_t *>(q), 0, nullptr,
                                            nullptr, 0, L, w0, fw);
    wave_lds_fence();
    unsigned long long best = 0;                                 // (fwd[a] - a) << 8 | 255 - (a - w0): the first maximum
    bool absent = false;
#pragma unroll
    for (int k = 0; k < kLrWin / kWave; k++) {
        const int t = k * kWave + lane, a = w0 + t;
        if (t < nw) {
            const int v = fw[t];
            __builtin_nontemporal_store(v, fwd + o + a);
            const unsigned long long key = ((unsigned long long)(uint32_t)(v - a) << kLrWinShift) | (unsigned)(kLrWin - 1 - t);
            best = key > best ? key : best;
            absent = absent || v == a;
            if (!MS && v < L) mark[o + v] = 1;                   // every writer stores the same value
        }
    }
    if (!MS) {
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const unsigned long long x = lr_shfl_xor64(best, m);
            best = x > best ? x : best;
        }
    }
    const bool any_absent = __any(absent);
    if (lane == 0) {
        if (!MS) wmax[gw] = make_int2((int)(best >> kLrWinShift), w0 + kLrWin - 1 - (int)(best & (kLrWin - 1)));
        if (any_absent) st[r] = GENIE_READ_ABSENT_BASE;
    }
}

template <bool SLICED>
__global__ void __launch_bounds__(kLrWin) lr_walk_kernel(int mode, int min_len, const long long *__restrict__ off, long long N,
                                                         const int32_t *__restrict__ st, const int32_t *__restrict__ fwd,
                                                         const int2 *__restrict__ wmax, const uint8_t *__restrict__ mark,
                                                         int32_t *__restrict__ bst, int2 *__restrict__ jc, long long win0)
{
    __shared__ int sJ[kLrWin], sC[kLrWin];
    __shared__ int32_t sf[2 * kLrWin];                         // fwd of the previous window and this one
    const long long gw = SLICED ? win0 + blockIdx.x : (long long)blockIdx.x;
    const long long r = lr_find(N, gw, [&](long long x) { return lr_wb(off, x); });
    const long long wb = lr_wb(off, r);
    const long long o = off[r], Ll = off[r + 1] - o;
    if (gw - wb < 0 || (gw - wb) * kLrWin >= Ll || st[r] != GENIE_READ_OK) return;      // block-uniform
    const int L = (int)Ll, w0 = (int)((gw - wb) * kLrWin);
    const int t = threadIdx.x, i = w0 + t;
    const int lim = L - w0 < kLrWin ? L : w0 + kLrWin;
    const bool marked = i < L && (i == 0 || mark[o + i]);
    const int32_t *f = fwd + o;
    const int lds0 = w0 - kLrWin;                                // most scans end inside the two windows staged in LDS
    for (int j = t; j < 2 * kLrWin; j += kLrWin) {
        const int p = lds0 + j;
        sf[j] = p >= 0 && p < L ? f[p] : 0;
    }
    __syncthreads();
    auto fv = [&](int p) { return p >= lds0 ? sf[p - lds0] : f[p]; };      // p <= i < L
    int J = lim, C = 0;
    if (marked) {
        int bl = 0, bb = i;
        for (int b = i; b >= 0;) {
            if ((b & (kLrWin - 1)) == kLrWin - 1 && fv(b - (kLrWin - 1)) > i) {   // the whole window [b - kLrWin + 1, b] covers i
                const int2 m = wmax[wb + (b >> kLrWinShift)];
                if (m.x >= bl) { bl = m.x; bb = m.y; }                           // going down: ties go to the smaller position
                b -= kLrWin;
                continue;
            }
            const int v = fv(b);
            if (v <= i) break;
            if (v - b >= bl) { bl = v - b; bb = b; }
            b--;
        }
        if (bl > 0) {
            J = bb + bl;
            C = (mode != GENIE_MODE_BWA || bl >= min_len) ? 1 : 0;
            bst[o + i] = bb;
        } else {
            J = L;                                               // read[i] occurs nowhere: the read is flagged (LR2)
        }
    }
    sJ[t] = J;
    sC[t] = C;
    __syncthreads();
    // an end inside the window is a value of fwd[], so it is marked and has its own step
    for (int round = 0; round < kLrWinShift; round++) {
        int nJ = J, nC = C;
        if (marked && J < lim) {
            nJ = sJ[J - w0];
            nC = C + sC[J - w0];
        }
        __syncthreads();
        J = nJ;
        C = nC;
        sJ[t] = J;
        sC[t] = C;
        __syncthreads();
    }
    if (marked) jc[o + i] = make_int2(J, C);
}

__global__ void __launch_bounds__(256) lr_chain_kernel(const long long *__restrict__ off, long long N, const int32_t *__restrict__ st,
                                                       const int2 *__restrict__ jc, int32_t *__restrict__ entry,
                                                       int32_t *__restrict__ base, int32_t *__restrict__ cnt)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const long long o = off[r];
    const int L = (int)(off[r + 1] - o);
    int total = 0;
    if (st[r] == GENIE_READ_OK && L > 0) {
        const long long wb = lr_wb(off, r);
        for (int e = 0; e < L;) {
            const long long g = wb + (e >> kLrWinShift);
            entry[g] = e;
            base[g] = total;
            const int2 v = jc[o + e];
            total += v.y;
            if (v.x <= e) break;                                 // cannot happen: every step leaves the window
            e = v.x;
        }
    }
    cnt[r] = total;
}

// ushift[u]: the unit's start inside its read, added to start / end of its rows; null: 0
__global__ void __launch_bounds__(256) lr_emit_kernel(DevIndex ix, int mode, int min_len, const long long *__restrict__ off, long long N,
                                                      long long nwin, const uint64_t *__restrict__ packed, const int32_t *__restrict__ fwd,
                                                      const int32_t *__restrict__ bst, const int32_t *__restrict__ entry,
                                                      const int32_t *__restrict__ base, const long long *__restrict__ offsets,
                                                      const int32_t *__restrict__ ushift, int4 *__restrict__ rows, long long cap)
{
    const long long gw = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= nwin) return;
    const int e = entry[gw];
    if (e < 0) return;                                           // a window the chain jumps over (or of a flagged unit)
    const long long r = lr_find(N, gw, [&](long long x) { return lr_wb(off, x); });
    const long long o = off[r];
    const int L = (int)(off[r + 1] - o);
    const int w0 = (int)((gw - lr_wb(off, r)) * kLrWin);
    const int lim = L - w0 < kLrWin ? L : w0 + kLrWin;
    const QPlain Q{packed + lr_wd(off, r)};
    const uint32_t sh = ushift ? (uint32_t)ushift[r] : 0u;
    long long k = offsets[r] + base[gw];
    for (int i = e; i < lim;) {
        const int b = bst[o + i], end = fwd[o + b];
        if (mode != GENIE_MODE_BWA || end - b >= min_len) {
            if (k < cap) {
                const int2 iv = sa_interval(ix, ix.dir, Q, b, end - b);
                store_nt(rows + k, make_uint4((uint32_t)b + sh, (uint32_t)end + sh, (uint32_t)iv.x, (uint32_t)iv.y));
            }
            k++;
        }
        i = end;
    }
}

typedef int lr_i2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void lr_store_lohi(int2 *dst, int2 iv)
{
    __builtin_nontemporal_store(lr_i2{iv.x, iv.y}, reinterpret_cast<lr_i2 *>(dst));
}

// LRM.  uvirt[u]: the virtual position (long_units.inc) of unit u's first base, where the unit's values go in ms / lohi; null:
// off[u].  lohi null: lengths only.  A unit with a bad base gets -1 and (-1, -1) everywhere.
template <bool C16, bool SLICED = false>
__global__ void __launch_bounds__(kLrWin) lr_ms_kernel(DevIndex ix, const long long *__restrict__ off, long long N,
                                                       const uint64_t *__restrict__ packed, const int32_t *__restrict__ st,
                                                       const int32_t *__restrict__ fwd, const long long *__restrict__ uvirt,
                                                       int32_t *__restrict__ ms, int2 *__restrict__ lohi, long long win0)
{
    __shared__ int32_t slen[kLrWin];
    __shared__ uint16_t slist[kLrWin];                           // the positions the entry does not decide
    __shared__ int nlist;
    const long long gw = SLICED ? win0 + blockIdx.x : (long long)blockIdx.x;
    const long long r = lr_find(N, gw, [&](long long x) { return lr_wb(off, x); });
    const long long w = gw - lr_wb(off, r);
    const long long o = off[r], Ll = off[r + 1] - o;
    if (w < 0 || w * kLrWin >= Ll) return;                     // block-uniform, as everything up to the first barrier
    const int L = (int)Ll, w0 = (int)(w * kLrWin);
    const int t = threadIdx.x, a = w0 + t, lane = t & (kWave - 1);
    const bool in = a < L;
    const long long v0 = (uvirt ? uvirt[r] : o) + w0;            // where the window's first position goes
    const bool bad = st[r] == GENIE_READ_BAD_BASE;
    const int len = in && !bad ? fwd[o + a] - a : -1;
    if (in) __builtin_nontemporal_store(len, ms + v0 + t);
    if (!lohi) return;
    if (bad) {
        if (in) lr_store_lohi(lohi + v0 + t, make_int2(-1, -1));
        return;
    }
    if (t == 0) nlist = 0;
    slen[t] = len;
    __syncthreads();
    const QPlain Q{packed + lr_wd(off, r)};
    const bool act = len > 0;
    const uint64_t x = act ? Q.win(a) : 0ull;
    int2 iv;                                                     // (-1, -1) where the match is empty
    const bool fast = interval_from_window<C16>(ix, x, len, act, iv);
    if (in && (fast || !act)) lr_store_lohi(lohi + v0 + t, iv);
    const bool general = act && !fast;
    const unsigned long long gb = __ballot(general);
    if (gb) {
        const int first = __ffsll((long long)gb) - 1;
        int at = 0;
        if (lane == first) at = atomicAdd(&nlist, __popcll(gb));
        at = __shfl(at, first, kWave);
        if (general) slist[at + __popcll(gb & ((1ull << lane) - 1ull))] = (uint16_t)t;
    }
    __syncthreads();
    if (t < nlist) {
        const int g = slist[t];
        const int2 v = sa_interval(ix, ix.dir, Q, w0 + g, slen[g]);
        lr_store_lohi(lohi + v0 + g, v);
    }
}

// The positions of the caller's arrays in front of the first read and behind the last one (the offsets need not begin at 0
// nor end at total_bases): no match.
__global__ void __launch_bounds__(256) lr_ms_edges_kernel(const long long *__restrict__ off, long long N, int S, long long positions,
                                                          int32_t *__restrict__ ms, int2 *__restrict__ lohi)
{
    const long long lead = S * off[0], tail = S * off[N];
    const long long n = lead + (positions - tail);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long v = i < lead ? i : tail + (i - lead);
        ms[v] = 0;
        if (lohi) lohi[v] = make_int2(-1, -1);
    }
}

struct LongArea {
    int *flag;
    int32_t *st, *cnt;
    uint8_t *sums;                   // launch_compact's scratch: nblocks + 1 words
    uint64_t *packed;
    int32_t *fwd, *bst;
    int2 *jc, *wmax;
    uint8_t *mark;
    int32_t *entry, *base;
    long long total, nwords, nwin;
};

// smems false: the pieces LR1 and LR2 use (the match-statistics tail), the others empty; fwd false as well: those of LR1
// alone (the exact-match tail)
inline int64_t long_layout(uint8_t *p, int64_t N, int64_t total, LongArea *a, bool smems = true, bool fwd = true)
{
    a->total = total;
    a->nwords = total / 32 + 3 * N + 4;
    a->nwin = total / kLrWin + N + 1;
    Carver c{p};
    c.take(a->flag, 256);
    c.take(a->st, 4 * N);
    c.take(a->cnt, smems ? 4 * N : 0);
    c.take(a->sums, 8 * ((N + kScanBlock - 1) / kScanBlock + 1));
    c.take(a->packed, 8 * a->nwords);
    c.take(a->fwd, fwd ? 4 * total : 0);
    c.take(a->bst, smems ? 4 * total : 0);
    c.take(a->jc, smems ? 8 * total : 0);
    c.take(a->mark, smems ? total : 0);
    c.take(a->wmax, smems ? 8 * a->nwin : 0);
    c.take(a->entry, smems ? 4 * a->nwin : 0);
    c.take(a->base, smems ? 4 * a->nwin : 0);
    return c.at;
}

// What a call may put between LR2 and whatever reads fwd[]: step(a, uoff, U) rewrites fwd[] of the U units in place
// (contig_stats.inc).  Empty: nothing.
using LrStep = std::function<int(const LongArea &, const long long *, long long)>;

// LR2's match-statistics instance over the U units of `uoff`: fwd[] alone, a.wmax and a.mark are not touched (below)
int lr_fwd_plain(const genie_index *ix, const LongArea &a, const long long *uoff, long long U, hipStream_t s);

// LR1 .. LR5 over the U units of `uoff`, the row counts to `offsets`: the one launch sequence of the long calls.  A step
// also rewrites a.wmax and a.mark from its fwd[], so the marks are cleared in front of it, not in front of LR2, and LR2
// writes neither where it need not: in BWA mode.  In LUT / RMI mode a read shorter than K keeps its status only in the
// SMEM instance, which skips it.
int lr_pipeline(const genie_index *ix, int mode, int min_len, const uint8_t *d_bases, const LongArea &a, const long long *uoff,
                long long U, const long long *usrc, const int32_t *ushift, int64_t *offsets, int32_t *d_rows, long long cap,
                const LrStep &step, hipStream_t s)
{
    HIP_TRY(hipMemsetAsync(a.entry, 0xFF, a.nwin * 4, s));
    if (a.total > 0 && !step) HIP_TRY(hipMemsetAsync(a.mark, 0, a.total, s));
    LAUNCH_BLOCKS(lr_pack_kernel, (a.nwords + 255) / 256, 256, 0, s, d_bases, uoff, U, usrc, a.nwords, a.packed, a.st);
    int rc = GENIE_OK;
    if (step && mode == GENIE_MODE_BWA) {
        if ((rc = lr_fwd_plain(ix, a, uoff, U, s))) return rc;
    } else {
        const bool c16 = (ix->dev.flags & kFlagCompactTable) != 0;
        const auto fwd_one = c16 ? lr_fwd_kernel<true> : lr_fwd_kernel<false>;
        const auto fwd_sliced = c16 ? lr_fwd_kernel<true, false, true> : lr_fwd_kernel<false, false, true>;
        LAUNCH_SLICED(fwd_one, fwd_sliced, (a.nwin + kLrFwdWaves - 1) / kLrFwdWaves, kLrFwdWaves * 64, 0, s, ix->dev, mode, uoff, U, a.nwin,
                      static_cast<const uint64_t *>(a.packed), a.st, a.fwd, a.wmax, a.mark, table_bytes(ix));
    }
    if (step) {
        if (a.total > 0) HIP_TRY(hipMemsetAsync(a.mark, 0, a.total, s));
        if ((rc = step(a, uoff, U))) return rc;
    }
    LAUNCH_SLICED(lr_walk_kernel<false>, lr_walk_kernel<true>, a.nwin, kLrWin, 0, s, mode, min_len, uoff, U,
                  static_cast<const int32_t *>(a.st), static_cast<const int32_t *>(a.fwd), static_cast<const int2 *>(a.wmax),
                  static_cast<const uint8_t *>(a.mark), a.bst, a.jc);
    LAUNCH_BLOCKS(lr_chain_kernel, (U + 255) / 256, 256, 0, s, uoff, U, a.st, a.jc, a.entry, a.base, a.cnt);
    if ((rc = launch_compact(a.cnt, nullptr, U, 0x7fffffff, offsets, nullptr, 0, a.sums, s))) return rc;
    LAUNCH_BLOCKS(lr_emit_kernel, (a.nwin + 255) / 256, 256, 0, s, ix->dev, mode, min_len, uoff, U, a.nwin, a.packed, a.fwd, a.bst,
                  a.entry, a.base, reinterpret_cast<const long long *>(offsets), ushift, reinterpret_cast<int4 *>(d_rows), cap);
    return GENIE_OK;
}

int lr_fwd_plain(const genie_index *ix, const LongArea &a, const long long *uoff, long long U, hipStream_t s)
{
    const bool c16 = (ix->dev.flags & kFlagCompactTable) != 0;
    const auto fwd_kernel = c16 ? lr_fwd_kernel<true, true> : lr_fwd_kernel<false, true>;
    const auto fwd_sliced = c16 ? lr_fwd_kernel<true, true, true> : lr_fwd_kernel<false, true, true>;
    LAUNCH_SLICED(fwd_kernel, fwd_sliced, (a.nwin + kLrFwdWaves - 1) / kLrFwdWaves, kLrFwdWaves * 64, 0, s, ix->dev, (int)GENIE_MODE_BWA, uoff, U,
                  a.nwin, static_cast<const uint64_t *>(a.packed), a.st, a.fwd, static_cast<int2 *>(nullptr),
                  static_cast<uint8_t *>(nullptr), table_bytes(ix));
    return GENIE_OK;
}

// LR1, LR2, the step and LRM over the U units of `uoff`: the matching statistics of every position of every unit to its
// place in ms / lohi (lohi may be null), the units' statuses to a.st
int lr_match_stats(const genie_index *ix, const uint8_t *d_bases, const LongArea &a, const long long *uoff, long long U,
                   const long long *usrc, const long long *uvirt, int32_t *d_ms, int32_t *d_lohi, const LrStep &step, hipStream_t s)
{
    LAUNCH_BLOCKS(lr_pack_kernel, (a.nwords + 255) / 256, 256, 0, s, d_bases, uoff, U, usrc, a.nwords, a.packed, a.st);
    int rc = lr_fwd_plain(ix, a, uoff, U, s);
    if (rc || (step && (rc = step(a, uoff, U)))) return rc;
    const bool c16 = (ix->dev.flags & kFlagCompactTable) != 0;
    const auto ms_kernel = c16 ? lr_ms_kernel<true> : lr_ms_kernel<false>;
    const auto ms_sliced = c16 ? lr_ms_kernel<true, true> : lr_ms_kernel<false, true>;
    LAUNCH_SLICED(ms_kernel, ms_sliced, a.nwin, kLrWin, 0, s, ix->dev, uoff, U, static_cast<const uint64_t *>(a.packed),
                  static_cast<const int32_t *>(a.st), static_cast<const int32_t *>(a.fwd), uvirt, d_ms, reinterpret_cast<int2 *>(d_lohi));
    return GENIE_OK;
}

}  // namespace

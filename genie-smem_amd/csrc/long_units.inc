// long_units.inc -- genie_find_smems_long, genie_find_smems_long_ex and genie_match_stats: how the units of long_reads.inc's
// pipelines are made from reads, strands and breaks, and the entry points (included by kernels.hip behind long_reads.inc,
// inside namespace genie).
//
// A unit is one strand of one segment of one read.  Strands and breaks are a property of the pack stage (usrc) and of
// where the rows land (ushift, the caller's offsets); everything between works on units alone.
//   strand-read q = S i + s   read i on strand s (S = 2 with GENIE_READS_BOTH_STRANDS, else 1); position p of a reversed
//                             strand-read is the read's position L - 1 - p, complemented (a code > 3 stays what it is)
//   virtual position          S off[i] + s L_i + p: the strand-reads back to back, [0, S total_bases)
//   LU0 lu_check_kernel       offsets non-decreasing, inside [0, total_bases], no read above max_len; the host reads the
//                             flag (the first synchronisation).  Also the status of every strand-read (too short for K in
//                             LUT / RMI mode) and, for two strands, the unit table of the strand-reads, empty ones
//                             included, with no pass over the bases.
//   The units are the strand-reads without GENIE_READS_SPLIT_BREAKS, or when its scan finds no break: lr_pipeline over
//   them, whose launch_compact writes the caller's offsets.  On one strand the caller's read offsets are the unit offsets
//   and there is no table, so nothing is copied; genie_find_smems_long is this case.
//   With GENIE_READS_SPLIT_BREAKS, parallel over positions (blocks of kLuChunk virtual positions across all strand-reads):
//   LU1 lu_seg_kernel<false>  good = code < 4 and present in the reference (split_present_bases); a segment starts where
//                             good and (previous not good or first of its strand-read).  A block stages one flag byte per
//                             position in LDS, a thread then takes kLuPer consecutive ones.  Starts per block, for every
//                             strand-read the starts of its block in front of its first position, and "a break exists".
//   scan_block_sums_kernel    over the block counts; the host reads the total and the break flag (the second
//                             synchronisation).
//   per pass of at most C consecutive units (C from the workspace, at least S N):
//   LU2 lu_seg_kernel<true>   the k-th start and the k-th end belong to the same segment: begin / end by rank
//   LU3 lu_units_kernel       length, first source byte, direction and start inside the strand-read of every unit
//   launch_compact            the unit lengths to uoff[]
//   lr_pipeline               over (uoff, C) with usrc and ushift, its rows behind those of the passes before
//   LU4 lu_offsets_kernel     a strand-read's offset is its first unit's (units of a strand-read are consecutive)
//   Between passes the host reads the pass's row total (one synchronisation per extra pass).
// genie_match_stats shares all of this up to the units of a pass (lu_run); in place of lr_pipeline and LU4 it runs
// lr_match_stats, which writes every position's values at its virtual position: ua[] of a segment, the offset of a strand-read.
// genie_exact_match (exact_match.inc) shares it too, never with GENIE_READS_SPLIT_BREAKS: its units are the strand-patterns.
namespace {

constexpr int kLuChunk = 16384;           // virtual positions per block of LU1 / LU2 ...
constexpr int kLuSub = 4096;              // ... taken kLuSub at a time,
constexpr int kLuPer = kLuSub / 256;      // kLuPer consecutive ones per thread
constexpr int kLuSpare = 32;              // with breaks the workspace holds one more unit per kLuSpare positions

struct LuReads {
    const uint8_t *bases;
    const long long *off;
    long long N;
    int S;
    __device__ __forceinline__ long long count() const { return N * S; }
    // first virtual position of strand-read q in [0, S N]
    __device__ __forceinline__ long long at(long long q) const
    {
        if (S == 1) return off[q];
        const long long o = off[q >> 1];
        return (q & 1) ? o + off[(q >> 1) + 1] : 2 * o;
    }
    __device__ __forceinline__ long long find(long long v) const
    {
        return lr_find(count(), v, [&](long long x) { return at(x); });
    }
};

// a unit's source: (index of its first base in strand order) * 2 + reversed
__device__ __forceinline__ long long lu_src_key(long long o, long long o2, bool rev, long long p)
{
    return rev ? (o2 - 1 - p) * 2 + 1 : (o + p) * 2;
}

// Every argument check that needs the offsets.  Given st: the status of every strand-read, 0 or GENIE_READ_TOO_SHORT (LUT /
// RMI mode, fewer than K bases -- empty reads too, as in K_A); LR1 overwrites it with GENIE_READ_BAD_BASE, which takes
// precedence.  Given uoff: the unit table (usrc, uoff) whose units are the strand-reads.
__global__ void __launch_bounds__(256) lu_check_kernel(const long long *__restrict__ off, long long N, long long total,
                                                       long long max_len, int mode, int K, int S, int *__restrict__ flag,
                                                       int32_t *__restrict__ st, long long *__restrict__ usrc,
                                                       long long *__restrict__ uoff)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > N) return;
    const long long o = off[r];
    bool bad = o < 0 || o > total;
    if (r < N) {
        const long long o2 = off[r + 1];
        bad = bad || o2 < o || o2 - o > max_len;
        const int32_t status = (mode != GENIE_MODE_BWA && o2 - o < K) ? GENIE_READ_TOO_SHORT : GENIE_READ_OK;
        for (int s = 0; s < S; s++) {
            const long long u = S * r + s;
            if (st) st[u] = status;
            if (uoff) {
                usrc[u] = lu_src_key(o, o2, s == 1, 0);
                uoff[u] = S == 1 ? o : (s ? o + o2 : 2 * o);
            }
        }
    } else if (uoff) {
        uoff[S * N] = S * o;
    }
    if (bad) atomicOr(flag, 1);
}

// flags of a virtual position: 1 good (no break), 2 first of its strand-read, 4 last of it, 8 inside the batch
struct LuSr {
    long long at, o, o2;            // first virtual position, source range of the read
    bool rev;
};

__device__ __forceinline__ LuSr lu_sr(const LuReads &R, long long q)
{
    const long long i = R.S == 1 ? q : q >> 1;
    LuSr s;
    s.o = R.off[i];
    s.o2 = R.off[i + 1];
    s.rev = R.S == 2 && (q & 1);
    s.at = R.S == 1 ? s.o : (s.rev ? s.o + s.o2 : 2 * s.o);
    return s;
}

__device__ __forceinline__ uint32_t lu_flags(const LuReads &R, uint32_t present, long long v, long long vlo, long long vhi,
                                             const LuSr &s0, const LuSr &s1)
{
    if (v < vlo || v >= vhi) return 0;
    LuSr s = s0;
    if (v < s.at || v >= s.at + (s.o2 - s.o)) {                  // not the block's first strand-read: the one behind it?
        s = s1;
        if (v < s.at || v >= s.at + (s.o2 - s.o)) s = lu_sr(R, R.find(v));
    }
    const long long p = v - s.at;
    const uint32_t c = R.bases[s.rev ? s.o2 - 1 - p : s.o + p];
    const bool good = c < 4u && ((present >> (c ^ (s.rev ? 3u : 0u))) & 1u);
    return (good ? 1u : 0u) | (p == 0 ? 2u : 0u) | (p == s.o2 - s.o - 1 ? 4u : 0u) | 8u;
}

// LU1 (SCATTER false) / LU2: a block stages the flags of kLuSub positions and of one neighbour on either side in LDS,
// then every thread takes kLuPer consecutive positions; one scan of the threads' start counts per kLuSub positions.
template <bool SCATTER>
__global__ void __launch_bounds__(256) lu_seg_kernel(DevIndex ix, LuReads R, unsigned long long *__restrict__ bsum,
                                                     int32_t *__restrict__ qloc, int *__restrict__ anybreak, long long p0,
                                                     long long p1, long long *__restrict__ ua, long long *__restrict__ ub)
{
#define LU_SEG_USABLE split_present_bases(ix)
#include "lu_seg_body.inc"
#undef LU_SEG_USABLE
}

// The same for a call with a minimum occurrence count (min_occ.inc): usable are the bases the reference holds that often
template <bool SCATTER>
__global__ void __launch_bounds__(256) lu_seg_occ_kernel(DevIndex ix, LuReads R, unsigned long long *__restrict__ bsum,
                                                         int32_t *__restrict__ qloc, int *__restrict__ anybreak, long long p0,
                                                         long long p1, long long *__restrict__ ua, long long *__restrict__ ub,
                                                         int min_occ)
{
#define LU_SEG_USABLE split_usable_bases(ix, min_occ)
#include "lu_seg_body.inc"
#undef LU_SEG_USABLE
}

// ua / ub: virtual begin / end of the pass's units.  Afterwards ub holds the unit's source key.
__global__ void __launch_bounds__(256) lu_units_kernel(LuReads R, long long C, const long long *__restrict__ ua,
                                                       long long *__restrict__ ub, int32_t *__restrict__ ulen,
                                                       int32_t *__restrict__ ushift)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= C) return;
    const long long vb = ua[j];
    const long long q = R.find(vb);
    const long long i = R.S == 1 ? q : q >> 1;
    const long long p = vb - R.at(q);
    ulen[j] = (int32_t)(ub[j] - vb);
    ushift[j] = (int32_t)p;
    ub[j] = lu_src_key(R.off[i], R.off[i + 1], R.S == 2 && (q & 1), p);
}

// strand-reads whose first unit is in the pass (or, in the last pass, that have none left) get their offset
__global__ void __launch_bounds__(256) lu_offsets_kernel(LuReads R, const unsigned long long *__restrict__ bsum,
                                                         const int32_t *__restrict__ qloc, long long units, long long p0,
                                                         long long p1, bool last, const long long *__restrict__ local_off,
                                                         long long row0, long long *__restrict__ offsets)
{
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long SN = R.count();
    if (q > SN) return;
    if (q == SN) {
        if (last) offsets[SN] = row0 + local_off[p1 - p0];
        return;
    }
    const int32_t loc = qloc[q];
    const long long f = loc < 0 ? units : (long long)bsum[R.at(q) / kLuChunk] + loc;
    if (f >= p0 && (f < p1 || (last && f == p1))) offsets[q] = row0 + local_off[f - p0];
}

// Workspace of the call.  With breaks first the segmentation's block counts and per-strand-read counts.  Then the area of C
// units: the pipeline's for C units and S total_bases positions -- it begins with the flag block (check flag, break flag),
// whose address therefore does not depend on C -- and behind it the pieces of the unit table that the units need: none
// for whole reads on one strand, source and offsets for strand-reads, all of them for segments.
struct LongExFixed {
    unsigned long long *bsum;        // blocks + 2 words
    int32_t *qloc;                   // S N + 1
    long long nblk;
};

inline int64_t long_ex_fixed_layout(uint8_t *p, int64_t N, int64_t total, int S, bool split, LongExFixed *f)
{
    f->nblk = split ? (S * total + kLuChunk - 1) / kLuChunk : 0;
    Carver c{p};
    c.take(f->bsum, split ? 8 * (f->nblk + 2) : 0);
    c.take(f->qloc, split ? 4 * (S * N + 1) : 0);
    return c.at;
}

struct LongExPass {
    LongArea lr;                     // long_layout(C, S total)
    long long *ua, *ub;              // C each: virtual begin, virtual end / source key
    int32_t *ulen, *ushift;
    long long *uoff, *loff;          // C + 1 each: unit offsets, the pass's row offsets
};

// smems false: the layout of the match-statistics tail (no rows: the pieces of LR3 .. LR5 and the row offsets are empty); fwd
// false as well: that of the exact-match tail (no fwd[] either)
inline int64_t long_ex_pass_layout(uint8_t *p, int64_t C, int64_t total, int S, bool split, LongExPass *a, bool smems = true,
                                   bool fwd = true)
{
    const bool table = S == 2 || split;
    Carver c{p, long_layout(p, C, S * total, &a->lr, smems, fwd)};
    c.take(a->ua, split ? 8 * C : 0);
    c.take(a->ub, table ? 8 * C : 0);
    c.take(a->ulen, split ? 4 * C : 0);
    c.take(a->ushift, split ? 4 * C : 0);
    c.take(a->uoff, table ? 8 * (C + 1) : 0);
    c.take(a->loff, split && smems ? 8 * (C + 1) : 0);
    return c.at;
}

// units the caller's workspace holds: the strand-reads (a table is laid out for one at least), with breaks one more per
// kLuSpare positions
inline int64_t long_ex_units(int64_t N, int64_t total, int S, bool split)
{
    return (S == 2 || split ? std::max<int64_t>(1, S * N) : N) + (split ? S * total / kLuSpare : 0);
}

inline int64_t long_ex_bytes(int64_t N, int64_t total_bases, int32_t flags, bool smems, bool fwd = true)
{
    const int S = (flags & GENIE_READS_BOTH_STRANDS) ? 2 : 1;
    const bool split = (flags & GENIE_READS_SPLIT_BREAKS) != 0;
    LongExFixed f;
    LongExPass a;
    return long_ex_fixed_layout(nullptr, N, total_bases, S, split, &f) +
           long_ex_pass_layout(nullptr, long_ex_units(N, total_bases, S, split), total_bases, S, split, &a, smems, fwd);
}

// Units per pass of lu_run when `avail` bytes follow the fixed part: as many as fit (at least S N: the caller sized the
// workspace for that many), and no more than the U there are.  Whoever sizes a piece by the units of a pass asks here too.
inline long long long_ex_pass_units(long long SN, long long U, int64_t total, int S, int64_t avail, bool smems, bool fwd)
{
    LongExPass a;
    return pass_size(std::max<long long>(SN, 1), U,
                     [&](long long c) { return long_ex_pass_layout(nullptr, c, total, S, true, &a, smems, fwd) <= avail; });
}

// One pass of at most C units, as the front hands it to a tail
struct LuPass {
    const LuReads &R;
    const LongExFixed &f;
    const LongExPass &a;
    long long U, p0, p1;             // units of the call; the pass holds the units [p0, p1)
};

// The front that genie_find_smems_long_ex and genie_match_stats share: everything up to "the units of this pass exist" (LU0,
// the strand-read table, LU1 .. LU3, the passes).  What is done with the units is the TAIL's:
//   tail.kSmems, tail.kFwd           which workspace layout the call has
//   tail.empty()                     N == 0
//   tail.whole(lr, uoff, usrc)       the units are the S N strand-reads (no SPLIT_BREAKS, or no break found); their statuses
//                                    are in lr.st
//   tail.broken(U)                   breaks exist and cut the strand-reads into U units (U may be 0): once, before the passes
//   tail.pass(p)                     the units [p0, p1): table in p.a (ua virtual begin, ub source key, ushift, uoff), p.a.lr.st zeroed
// min_occ: a base counts as usable (no break, with GENIE_READS_SPLIT_BREAKS) when the reference holds it that often; 1, the
// default, is "present in the reference" and launches the kernels as ever.
template <class Tail>
int lu_run(const genie_index *ix, int32_t mode, const CsrBatch &b, hipStream_t s, Tail &tail, int32_t min_occ = 1)
{
    if (b.N == 0) return tail.empty();
    const int64_t N = b.N, total_bases = b.total_bases;
    const int S = b.strands();
    const bool split = b.split();
    const long long SN = b.strand_reads();
    const long long *off = reinterpret_cast<const long long *>(b.read_offsets);
    LongExFixed f;
    const int64_t fixed = long_ex_fixed_layout(static_cast<uint8_t *>(b.ws), N, total_bases, S, split, &f);
    uint8_t *pass = static_cast<uint8_t *>(b.ws) + fixed;
    // The strand-reads as units.  On one strand the caller's offsets are the unit offsets and there is no table.
    LongExPass whole;
    long_ex_pass_layout(pass, SN, total_bases, S, false, &whole, Tail::kSmems, Tail::kFwd);
    int *const flag = whole.lr.flag;
    long long *const tsrc = S == 2 ? whole.ub : nullptr, *const toff = S == 2 ? whole.uoff : nullptr;
    HIP_TRY(hipMemsetAsync(flag, 0, 8, s));
    LAUNCH_BLOCKS(lu_check_kernel, (N + 1 + 255) / 256, 256, 0, s, off, (long long)N, (long long)total_bases,
           (long long)b.max_len, mode, ix->dev.K, S, flag, whole.lr.st, tsrc, toff);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return GENIE_E_INVALID;
    if (!split) return tail.whole(whole.lr, toff ? toff : off, tsrc);

    const LuReads R{b.bases, off, (long long)N, S};
    int *anybreak = flag + 1;
    HIP_TRY(hipMemsetAsync(f.qloc, 0xFF, (SN + 1) * 4, s));
    if (f.nblk > 0 && min_occ > 1)
        LAUNCH_BLOCKS(lu_seg_occ_kernel<false>, f.nblk, 256, 0, s, ix->dev, R, f.bsum, f.qloc, anybreak, 0ll, 0ll,
               static_cast<long long *>(nullptr), static_cast<long long *>(nullptr), (int)min_occ);
    else if (f.nblk > 0)
        LAUNCH_BLOCKS(lu_seg_kernel<false>, f.nblk, 256, 0, s, ix->dev, R, f.bsum, f.qloc, anybreak, 0ll, 0ll,
               static_cast<long long *>(nullptr), static_cast<long long *>(nullptr));
    LAUNCH(scan_block_sums_kernel, dim3(1), dim3(kScanBlock), 0, s, f.bsum, f.nblk);
    unsigned long long units = 0;
    int breaks = 0;
    HIP_TRY(hipMemcpyAsync(&units, f.bsum + f.nblk, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&breaks, anybreak, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!breaks) return tail.whole(whole.lr, toff ? toff : off, tsrc);      // every status is GENIE_READ_OK: BWA mode, no bad or absent base
    const long long U = (long long)units;
    int rc = tail.broken(U);
    if (rc || U == 0) return rc;
    LongExPass a;
    const long long C = long_ex_pass_units(SN, U, total_bases, S, b.ws_bytes - fixed, Tail::kSmems, Tail::kFwd);
    long_ex_pass_layout(pass, C, total_bases, S, true, &a, Tail::kSmems, Tail::kFwd);
    for (long long p0 = 0; p0 < U; p0 += C) {
        const long long p1 = std::min(U, p0 + C), Cp = p1 - p0;
        HIP_TRY(hipMemsetAsync(a.lr.st, 0, Cp * 4, s));           // GENIE_READ_OK: a unit holds no break
        if (min_occ > 1)
            LAUNCH_BLOCKS(lu_seg_occ_kernel<true>, f.nblk, 256, 0, s, ix->dev, R, f.bsum, f.qloc, anybreak, p0, p1, a.ua, a.ub,
                          (int)min_occ);
        else
            LAUNCH_BLOCKS(lu_seg_kernel<true>, f.nblk, 256, 0, s, ix->dev, R, f.bsum, f.qloc, anybreak, p0, p1, a.ua, a.ub);
        LAUNCH_BLOCKS(lu_units_kernel, (Cp + 255) / 256, 256, 0, s, R, Cp, static_cast<const long long *>(a.ua), a.ub,
               a.ulen, a.ushift);
        rc = launch_compact(a.ulen, nullptr, Cp, 0x7fffffff, reinterpret_cast<int64_t *>(a.uoff), nullptr, 0, a.lr.sums, s);
        if (rc) return rc;
        if ((rc = tail.pass(LuPass{R, f, a, U, p0, p1}))) return rc;
    }
    return GENIE_OK;
}

// The SMEM tail: lr_pipeline over the units, then LU4.  Between passes the host reads the pass's row total.
struct LuSmemTail {
    static constexpr bool kSmems = true, kFwd = true;
    const genie_index *ix;
    int32_t mode, min_len;
    const CsrBatch &b;
    const CsrRows &out;
    hipStream_t s;
    LrStep step;                     // between LR2 and LR3 (long_reads.inc), or empty
    long long row0 = 0;              // rows of the passes before

    int empty()
    {
        HIP_TRY(hipMemsetAsync(out.offsets, 0, 8, s));
        return GENIE_OK;
    }
    int whole(const LongArea &lr, const long long *uoff, const long long *usrc)
    {
        const long long SN = b.strand_reads();
        int rc = lr_pipeline(ix, mode, min_len, b.bases, lr, uoff, SN, usrc, nullptr, out.offsets, out.rows, out.cap_rows, step, s);
        if (rc) return rc;
        if (b.status) HIP_TRY(hipMemcpyAsync(b.status, lr.st, SN * 4, hipMemcpyDeviceToDevice, s));
        return GENIE_OK;
    }
    int broken(long long U)
    {
        const long long SN = b.strand_reads();
        if (b.status) HIP_TRY(hipMemsetAsync(b.status, 0, SN * 4, s));
        if (U == 0) HIP_TRY(hipMemsetAsync(out.offsets, 0, (SN + 1) * 8, s));
        return GENIE_OK;
    }
    int pass(const LuPass &p)
    {
        const LongExPass &a = p.a;
        const long long SN = b.strand_reads(), Cp = p.p1 - p.p0;
        const bool last = p.p1 == p.U;
        const long long cap_left = std::max(0ll, (long long)out.cap_rows - row0);
        int rc = lr_pipeline(ix, mode, min_len, b.bases, a.lr, a.uoff, Cp, a.ub, a.ushift, reinterpret_cast<int64_t *>(a.loff),
                             cap_left > 0 ? out.rows + 4 * row0 : out.rows, cap_left, step, s);
        if (rc) return rc;
        LAUNCH_BLOCKS(lu_offsets_kernel, (SN + 1 + 255) / 256, 256, 0, s, p.R, static_cast<const unsigned long long *>(p.f.bsum),
               static_cast<const int32_t *>(p.f.qloc), p.U, p.p0, p.p1, last, static_cast<const long long *>(a.loff), row0,
               reinterpret_cast<long long *>(out.offsets));
        if (!last) {
            long long pass_rows = 0;
            HIP_TRY(hipMemcpyAsync(&pass_rows, a.loff + Cp, 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            row0 += pass_rows;
        }
        return GENIE_OK;
    }
};

// The match-statistics tail: lr_match_stats over the units.  Positions that no unit covers (breaks; what lies in front of the
// first read and behind the last) are filled beforehand; nothing is read back between passes.
struct LuMsTail {
    static constexpr bool kSmems = false, kFwd = true;
    const genie_index *ix;
    const CsrBatch &b;
    int32_t *d_ms, *d_lohi;
    hipStream_t s;
    LrStep step;                     // between LR2 and LRM (long_reads.inc), or empty

    int fill()                       // no match anywhere
    {
        const long long positions = b.positions();
        if (positions > 0) HIP_TRY(hipMemsetAsync(d_ms, 0, positions * 4, s));
        if (positions > 0 && d_lohi) HIP_TRY(hipMemsetAsync(d_lohi, 0xFF, positions * 8, s));
        return GENIE_OK;
    }
    int empty() { return fill(); }
    int whole(const LongArea &lr, const long long *uoff, const long long *usrc)
    {
        const long long SN = b.strand_reads();
        LAUNCH(lr_ms_edges_kernel, dim3(64), dim3(256), 0, s, reinterpret_cast<const long long *>(b.read_offsets), (long long)b.N,
               b.strands(), b.positions(), d_ms, reinterpret_cast<int2 *>(d_lohi));
        int rc = lr_match_stats(ix, b.bases, lr, uoff, SN, usrc, nullptr, d_ms, d_lohi, step, s);     // a strand-read's offset is its virtual position
        if (rc) return rc;
        if (b.status) HIP_TRY(hipMemcpyAsync(b.status, lr.st, SN * 4, hipMemcpyDeviceToDevice, s));
        return GENIE_OK;
    }
    int broken(long long)
    {
        if (b.status) HIP_TRY(hipMemsetAsync(b.status, 0, b.strand_reads() * 4, s));
        return fill();
    }
    int pass(const LuPass &p)
    {
        return lr_match_stats(ix, b.bases, p.a.lr, p.a.uoff, p.p1 - p.p0, p.a.ub, p.a.ua, d_ms, d_lohi, step, s);
    }
};

}  // namespace

int64_t find_smems_long_ex_workspace_bytes(int64_t N, int64_t total_bases, int32_t flags)
{
    return long_ex_bytes(N, total_bases, flags, true);
}

int launch_find_smems_long_ex(const genie_index *ix, int32_t mode, int32_t min_len, const CsrBatch &b, const CsrRows &out, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    LuSmemTail tail{ix, mode, min_len, b, out, s};
    return lu_run(ix, mode, b, s, tail);
}

int64_t match_stats_workspace_bytes(int64_t N, int64_t total_bases, int32_t flags)
{
    return long_ex_bytes(N, total_bases, flags, false);
}

int launch_match_stats(const genie_index *ix, const CsrBatch &b, int32_t *d_ms, int32_t *d_lohi, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    LuMsTail tail{ix, b, d_ms, d_lohi, s};
    return lu_run(ix, GENIE_MODE_BWA, b, s, tail);
}

// long_units.inc -- genie_find_smems_long_ex: both strands and breaks for reads of any length (included by kernels.hip
// behind long_reads.inc, inside namespace genie; uses its kernels and layout).
//
// Of the long-read pipeline only the pack stage reads the caller's bases; LR2 .. LR5 work on the packed stream and on
// workspace rows addressed through the offsets array they are handed.  So the pipeline is handed UNITS instead of reads:
// a unit is one strand of one segment of one read, and uoff[U + 1] (prefix sums of the unit lengths) takes the place of
// the read offsets.  Strands and breaks are then a property of the pack stage and of where the rows land.
//   strand-read q = S i + s   read i on strand s (S = 2 with GENIE_READS_BOTH_STRANDS, else 1); position p of a reversed
//                             strand-read is the read's position L - 1 - p, complemented (a code > 3 stays what it is)
//   virtual position          S off[i] + s L_i + p: the strand-reads back to back, [0, S total_bases)
//   LU0 lu_check_kernel       LR0's offset check (the host reads the flag: the first synchronisation).  Without breaks it
//                             also writes the unit table -- the units are the strand-reads, empty ones included -- with
//                             no pass over the bases.
//   with GENIE_READS_SPLIT_BREAKS, parallel over positions (blocks of kLuChunk virtual positions across all strand-reads):
//   LU1 lu_seg_kernel<false>  good = code < 4 and present in the reference (split_present_bases); a segment starts where
//                             good and (previous not good or first of its strand-read).  A block stages one flag byte per
//                             position in LDS, a thread then takes kLuPer consecutive ones.  Starts per block, for every
//                             strand-read the starts of its block in front of its first position, and "a break exists".
//   scan_block_sums_kernel    over the block counts; the host reads the total and the break flag (the second
//                             synchronisation).  No break anywhere: the units are the strand-reads, as without the flag.
//   per pass of at most C consecutive units (C from the workspace, at least S N):
//   LU2 lu_seg_kernel<true>   the k-th start and the k-th end belong to the same segment: begin / end by rank
//   LU3 lu_units_kernel       length, first source byte, direction and start inside the strand-read of every unit
//   launch_compact            the unit lengths to uoff[]
//   LU4 lu_pack_kernel        LR1 for units: one thread per 64-bit word; a reversed unit is read backwards and complemented
//                             after the bad-base test on the raw bytes.  The reverse complement is never written as bytes.
//   LR2 .. LR4, launch_compact   unchanged, over (uoff, U)
//   LU5 lu_emit_kernel        LR5 with the unit's start added where the row is written (every row written once)
//   LU6 lu_offsets_kernel     a strand-read's offset is its first unit's (units of a strand-read are consecutive)
//   Between passes the host reads the pass's row total (one synchronisation per extra pass).
// Without breaks LR5 itself emits and launch_compact writes the caller's offsets: one synchronisation, as the long call.
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

__global__ void __launch_bounds__(256) lu_check_kernel(const long long *__restrict__ off, long long N, long long total,
                                                       long long max_len, int mode, int K, int S, bool table, int *__restrict__ flag,
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
        if (table) {
            const int32_t status = (mode != GENIE_MODE_BWA && o2 - o < K) ? GENIE_READ_TOO_SHORT : GENIE_READ_OK;
            for (int s = 0; s < S; s++) {
                const long long u = S * r + s;
                st[u] = status;
                usrc[u] = lu_src_key(o, o2, s == 1, 0);
                uoff[u] = S == 1 ? o : (s ? o + o2 : 2 * o);
            }
        }
    } else if (table) {
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
    __shared__ uint8_t sflag[kLuSub + 8];
    __shared__ int wtot[4];
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t >> 6;
    const long long c0 = (long long)blockIdx.x * kLuChunk;
    long long run = 0;                                           // starts in front of the current kLuSub positions
    if (SCATTER) {
        const long long a = (long long)bsum[blockIdx.x], b = (long long)bsum[blockIdx.x + 1];
        if (b <= p0 || a > p1) return;                           // block-uniform: no unit of the pass begins or ends here
        run = a;
    }
    const uint32_t present = split_present_bases(ix);
    const long long vlo = R.at(0), vhi = R.at(R.count());
    long long q0 = R.find(c0);
    LuSr s0 = lu_sr(R, q0), s1 = lu_sr(R, q0 + 1 < R.count() ? q0 + 1 : q0);
    bool brk = false;
    for (int sub = 0; sub < kLuChunk / kLuSub; sub++) {
        const long long cs = c0 + sub * kLuSub;
        if (cs >= vhi) break;                                    // block-uniform
        if (cs >= s0.at + (s0.o2 - s0.o)) {
            q0 = R.find(cs);
            s0 = lu_sr(R, q0);
            s1 = lu_sr(R, q0 + 1 < R.count() ? q0 + 1 : q0);
        }
        const long long len0 = s0.o2 - s0.o, pb = cs - 1 - s0.at;
        if (pb >= 0 && pb + kLuSub + 2 <= len0) {                // all inside one strand-read (block-uniform): 32-bit work only
            const uint8_t *b0 = R.bases + (s0.rev ? s0.o2 - 1 - pb : s0.o + pb);
            const int jf = pb == 0 ? 0 : -1, jl = len0 - 1 - pb <= kLuSub + 1 ? (int)(len0 - 1 - pb) : -1;
            const uint32_t x = s0.rev ? 3u : 0u;
            for (int j = t; j < kLuSub + 2; j += 256) {
                const uint32_t c = s0.rev ? b0[-j] : b0[j];
                const bool good = c < 4u && ((present >> (c ^ x)) & 1u);
                sflag[j] = (uint8_t)((good ? 1u : 0u) | (j == jf ? 2u : 0u) | (j == jl ? 4u : 0u) | 8u);
            }
        } else {
            for (int j = t; j < kLuSub + 2; j += 256) sflag[j] = (uint8_t)lu_flags(R, present, cs - 1 + j, vlo, vhi, s0, s1);
        }
        __syncthreads();
        uint32_t f[kLuPer + 2];
#pragma unroll
        for (int i = 0; i < kLuPer + 2; i++) f[i] = sflag[kLuPer * t + i];
        uint32_t sm = 0, em = 0;
#pragma unroll
        for (int i = 0; i < kLuPer; i++) {
            const uint32_t cur = f[i + 1];
            const bool g = cur & 1u;
            if (g && ((cur & 2u) || !(f[i] & 1u))) sm |= 1u << i;
            if (g && ((cur & 4u) || !(f[i + 2] & 1u))) em |= 1u << i;
            brk = brk || (cur & 9u) == 8u;
        }
        const int cnt = __popc(sm);
        int inc = cnt;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int x = __shfl_up(inc, o, kWave);
            if (lane >= o) inc += x;
        }
        if (lane == kWave - 1) wtot[wave] = inc;
        __syncthreads();
        int all = 0;
        long long seen = run + inc - cnt;                        // starts in front of the thread's positions
        for (int w = 0; w < 4; w++) {
            const int x = wtot[w];
            seen += w < wave ? x : 0;
            all += x;
        }
        const long long v0 = cs + kLuPer * t;
        if (!SCATTER) {
#pragma unroll
            for (int i = 0; i < kLuPer; i++) {
                if (f[i + 1] & 2u) {                             // a strand-read begins: also the empty ones that sit here
                    const long long v = v0 + i;
                    const int32_t loc = (int32_t)(seen + __popc(sm & ((1u << i) - 1u)));
                    const long long q = R.find(v);
                    qloc[q] = loc;
                    for (long long e = q - 1; e >= 0 && R.at(e) == v; e--) qloc[e] = loc;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < kLuPer; i++) {
                if ((sm >> i) & 1u) seen++;
                const long long k = seen - 1;                    // the segment a good position belongs to
                if (k >= p0 && k < p1) {
                    if ((sm >> i) & 1u) ua[k - p0] = v0 + i;
                    if ((em >> i) & 1u) ub[k - p0] = v0 + i + 1;
                }
            }
        }
        run += all;
        __syncthreads();
    }
    if (!SCATTER) {
        // one writer per block, and none once the flag is up
        if (__syncthreads_or(brk) && t == 0 && __hip_atomic_load(anybreak, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
            atomicOr(anybreak, 1);
        if (t == 0) bsum[blockIdx.x] = (unsigned long long)run;
    }
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

__global__ void __launch_bounds__(256) lu_pack_kernel(const uint8_t *__restrict__ bases, const long long *__restrict__ uoff, long long U,
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
        const long long key = usrc[u];
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

// LR5 with the unit's start inside its strand-read added to start / end
__global__ void __launch_bounds__(256) lu_emit_kernel(DevIndex ix, int mode, int min_len, const long long *__restrict__ off, long long N,
                                                      long long nwin, const uint64_t *__restrict__ packed, const int32_t *__restrict__ fwd,
                                                      const int32_t *__restrict__ bst, const int32_t *__restrict__ entry,
                                                      const int32_t *__restrict__ base, const long long *__restrict__ offsets,
                                                      const int32_t *__restrict__ ushift, int4 *__restrict__ rows, long long cap)
{
    const long long gw = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= nwin) return;
    const int e = entry[gw];
    if (e < 0) return;
    const long long r = lr_find(N, gw, [&](long long x) { return lr_wb(off, x); });
    const long long o = off[r];
    const int L = (int)(off[r + 1] - o);
    const int w0 = (int)((gw - lr_wb(off, r)) * kLrWin);
    const int lim = L - w0 < kLrWin ? L : w0 + kLrWin;
    const QPlain Q{packed + lr_wd(off, r)};
    const uint32_t sh = (uint32_t)ushift[r];
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

// Workspace of the call: the check flag, the segmentation's block counts and per-strand-read counts, then a pass area
// for C units: the unit table and the long-read pipeline for C units and S total_bases positions.
struct LongExFixed {
    int *flag;
    unsigned long long *bsum;        // blocks + 2 words
    int32_t *qloc;                   // S N + 1
    long long nblk;
};

inline int64_t long_ex_fixed_layout(uint8_t *p, int64_t N, int64_t total, int S, bool split, LongExFixed *f)
{
    f->nblk = split ? (S * total + kLuChunk - 1) / kLuChunk : 0;
    Carver c{p};
    c.take(f->flag, 256);
    c.take(f->bsum, split ? 8 * (f->nblk + 2) : 0);
    c.take(f->qloc, split ? 4 * (S * N + 1) : 0);
    return c.at;
}

struct LongExPass {
    long long *ua, *ub;              // C each: virtual begin, virtual end / source key
    int32_t *ulen, *ushift;
    long long *uoff, *loff;          // C + 1 each: unit offsets, the pass's row offsets
    uint8_t *lr;                     // long_layout(C, S total)
};

inline int64_t long_ex_pass_layout(uint8_t *p, int64_t C, int64_t vtotal, bool split, LongExPass *a)
{
    Carver c{p};
    c.take(a->ua, split ? 8 * C : 0);
    c.take(a->ub, 8 * C);
    c.take(a->ulen, split ? 4 * C : 0);
    c.take(a->ushift, split ? 4 * C : 0);
    c.take(a->uoff, 8 * (C + 1));
    c.take(a->loff, split ? 8 * (C + 1) : 0);
    c.take(a->lr, 0);
    LongArea la;
    return c.at + long_layout(nullptr, C, vtotal, &la);
}

// LU4, LR2 .. LR4 and the row counts to `offsets`, then LR5 (ushift null) or LU5
int lu_pipeline(const genie_index *ix, int mode, int min_len, const uint8_t *d_bases, const LongArea &a, const long long *uoff,
                long long U, const long long *usrc, const int32_t *ushift, int64_t *offsets, int32_t *d_rows, long long cap,
                hipStream_t s)
{
    LAUNCH(lu_pack_kernel, dim3((unsigned)((a.nwords + 255) / 256)), dim3(256), 0, s, d_bases, uoff, U, usrc, a.nwords, a.packed, a.st);
    const dim3 fgrid((unsigned)((a.nwin + kLrFwdWaves - 1) / kLrFwdWaves)), fblock(kLrFwdWaves * 64);
    if (ix->dev.flags & kFlagCompactTable)
        LAUNCH(lr_fwd_kernel<true>, fgrid, fblock, 0, s, ix->dev, mode, uoff, U, a.nwin, a.packed, a.st, a.fwd, a.wmax, a.mark,
               table_bytes(ix));
    else
        LAUNCH(lr_fwd_kernel<false>, fgrid, fblock, 0, s, ix->dev, mode, uoff, U, a.nwin, a.packed, a.st, a.fwd, a.wmax, a.mark,
               table_bytes(ix));
    LAUNCH(lr_walk_kernel, dim3((unsigned)a.nwin), dim3(kLrWin), 0, s, mode, min_len, uoff, U, a.st, a.fwd, a.wmax, a.mark, a.bst,
           a.jc);
    LAUNCH(lr_chain_kernel, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, s, uoff, U, a.st, a.jc, a.entry, a.base, a.cnt);
    int rc = launch_compact(a.cnt, nullptr, U, 0x7fffffff, offsets, nullptr, 0, a.sums, s);
    if (rc) return rc;
    const dim3 egrid((unsigned)((a.nwin + 255) / 256));
    if (ushift)
        LAUNCH(lu_emit_kernel, egrid, dim3(256), 0, s, ix->dev, mode, min_len, uoff, U, a.nwin, a.packed, a.fwd, a.bst, a.entry, a.base,
               reinterpret_cast<const long long *>(offsets), ushift, reinterpret_cast<int4 *>(d_rows), cap);
    else
        LAUNCH(lr_emit_kernel, egrid, dim3(256), 0, s, ix->dev, mode, min_len, uoff, U, a.nwin, a.packed, a.fwd, a.bst, a.entry, a.base,
               reinterpret_cast<const long long *>(offsets), reinterpret_cast<int4 *>(d_rows), cap);
    return GENIE_OK;
}

inline int64_t long_ex_units(int64_t N, int64_t total, int S, bool split)
{
    return std::max<int64_t>(1, S * N) + (split ? S * total / kLuSpare : 0);
}

}  // namespace

int64_t find_smems_long_ex_workspace_bytes(int64_t N, int64_t total_bases, int32_t flags)
{
    if (flags == 0) return find_smems_long_workspace_bytes(N, total_bases);
    const int S = (flags & GENIE_READS_BOTH_STRANDS) ? 2 : 1;
    const bool split = (flags & GENIE_READS_SPLIT_BREAKS) != 0;
    LongExFixed f;
    LongExPass a;
    return long_ex_fixed_layout(nullptr, N, total_bases, S, split, &f) +
           long_ex_pass_layout(nullptr, long_ex_units(N, total_bases, S, split), S * total_bases, split, &a);
}

int launch_find_smems_long_ex(const genie_index *ix, int32_t mode, int32_t flags, const uint8_t *d_bases, const int64_t *d_read_offsets,
                              int64_t N, int64_t total_bases, int64_t max_len, int32_t min_len, int64_t *d_offsets, int32_t *d_rows,
                              int64_t out_cap_rows, int32_t *d_status, void *d_ws, int64_t ws_bytes, void *stream)
{
    if (flags == 0)
        return launch_find_smems_long(ix, mode, d_bases, d_read_offsets, N, total_bases, max_len, min_len, d_offsets, d_rows,
                                      out_cap_rows, d_status, d_ws, ws_bytes, stream);
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, 8, s));
        return GENIE_OK;
    }
    const int S = (flags & GENIE_READS_BOTH_STRANDS) ? 2 : 1;
    const bool split = (flags & GENIE_READS_SPLIT_BREAKS) != 0;
    const long long SN = (long long)S * N, vtotal = (long long)S * total_bases;
    const long long *off = reinterpret_cast<const long long *>(d_read_offsets);
    LongExFixed f;
    const int64_t fixed = long_ex_fixed_layout(static_cast<uint8_t *>(d_ws), N, total_bases, S, split, &f);
    uint8_t *pass = static_cast<uint8_t *>(d_ws) + fixed;
    LongExPass a;
    LongArea la;
    if (!split) {
        long_ex_pass_layout(pass, SN, vtotal, false, &a);
        long_layout(a.lr, SN, vtotal, &la);
    }
    HIP_TRY(hipMemsetAsync(f.flag, 0, 8, s));
    LAUNCH(lu_check_kernel, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, s, off, (long long)N, (long long)total_bases,
           (long long)max_len, mode, ix->dev.K, S, !split, f.flag, split ? nullptr : la.st, split ? nullptr : a.ub,
           split ? nullptr : a.uoff);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, f.flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return GENIE_E_INVALID;

    if (!split) {                                                // the units are the strand-reads
        HIP_TRY(hipMemsetAsync(la.entry, 0xFF, la.nwin * 4, s));
        if (vtotal > 0) HIP_TRY(hipMemsetAsync(la.mark, 0, vtotal, s));
        int rc = lu_pipeline(ix, mode, min_len, d_bases, la, a.uoff, SN, a.ub, nullptr, d_offsets, d_rows, out_cap_rows, s);
        if (rc) return rc;
        if (d_status) HIP_TRY(hipMemcpyAsync(d_status, la.st, SN * 4, hipMemcpyDeviceToDevice, s));
        return GENIE_OK;
    }

    const LuReads R{d_bases, off, (long long)N, S};
    int *anybreak = f.flag + 1;
    HIP_TRY(hipMemsetAsync(f.qloc, 0xFF, (SN + 1) * 4, s));
    if (f.nblk > 0)
        LAUNCH(lu_seg_kernel<false>, dim3((unsigned)f.nblk), dim3(256), 0, s, ix->dev, R, f.bsum, f.qloc, anybreak, 0ll, 0ll,
               static_cast<long long *>(nullptr), static_cast<long long *>(nullptr));
    LAUNCH(scan_block_sums_kernel, dim3(1), dim3(kScanBlock), 0, s, f.bsum, f.nblk);
    unsigned long long units = 0;
    int breaks = 0;
    HIP_TRY(hipMemcpyAsync(&units, f.bsum + f.nblk, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&breaks, anybreak, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (d_status) HIP_TRY(hipMemsetAsync(d_status, 0, SN * 4, s));
    if (!breaks) {                                               // no break anywhere: the units are the strand-reads
        long_ex_pass_layout(pass, SN, vtotal, false, &a);
        long_layout(a.lr, SN, vtotal, &la);
        LAUNCH(lu_check_kernel, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, s, off, (long long)N, (long long)total_bases,
               (long long)max_len, mode, ix->dev.K, S, true, f.flag, la.st, a.ub, a.uoff);
        HIP_TRY(hipMemsetAsync(la.entry, 0xFF, la.nwin * 4, s));
        if (vtotal > 0) HIP_TRY(hipMemsetAsync(la.mark, 0, vtotal, s));
        return lu_pipeline(ix, mode, min_len, d_bases, la, a.uoff, SN, a.ub, nullptr, d_offsets, d_rows, out_cap_rows, s);
    }
    const long long U = (long long)units;
    if (U == 0) {
        HIP_TRY(hipMemsetAsync(d_offsets, 0, (SN + 1) * 8, s));
        return GENIE_OK;
    }
    // units per pass: as many as the workspace holds (at least S N: the caller sized it for that many)
    long long C = std::max<long long>(SN, 1);
    {
        long long lo = C, hi = std::max(C, U);
        while (lo < hi) {
            const long long mid = lo + (hi - lo + 1) / 2;
            if (long_ex_pass_layout(nullptr, mid, vtotal, true, &a) <= ws_bytes - fixed) lo = mid; else hi = mid - 1;
        }
        C = std::min(lo, U);
    }
    long_ex_pass_layout(pass, C, vtotal, true, &a);
    long_layout(a.lr, C, vtotal, &la);
    long long row0 = 0;
    for (long long p0 = 0; p0 < U; p0 += C) {
        const long long p1 = std::min(U, p0 + C), Cp = p1 - p0;
        const bool last = p1 == U;
        HIP_TRY(hipMemsetAsync(la.st, 0, Cp * 4, s));             // GENIE_READ_OK: a unit holds no break
        HIP_TRY(hipMemsetAsync(la.entry, 0xFF, la.nwin * 4, s));
        HIP_TRY(hipMemsetAsync(la.mark, 0, vtotal, s));
        LAUNCH(lu_seg_kernel<true>, dim3((unsigned)f.nblk), dim3(256), 0, s, ix->dev, R, f.bsum, f.qloc, anybreak, p0, p1, a.ua, a.ub);
        LAUNCH(lu_units_kernel, dim3((unsigned)((Cp + 255) / 256)), dim3(256), 0, s, R, Cp, static_cast<const long long *>(a.ua), a.ub,
               a.ulen, a.ushift);
        int rc = launch_compact(a.ulen, nullptr, Cp, 0x7fffffff, reinterpret_cast<int64_t *>(a.uoff), nullptr, 0, la.sums, stream);
        if (rc) return rc;
        const long long cap_left = std::max(0ll, (long long)out_cap_rows - row0);
        rc = lu_pipeline(ix, mode, min_len, d_bases, la, a.uoff, Cp, a.ub, a.ushift, reinterpret_cast<int64_t *>(a.loff),
                         cap_left > 0 ? d_rows + 4 * row0 : d_rows, cap_left, s);
        if (rc) return rc;
        LAUNCH(lu_offsets_kernel, dim3((unsigned)((SN + 1 + 255) / 256)), dim3(256), 0, s, R, static_cast<const unsigned long long *>(f.bsum),
               static_cast<const int32_t *>(f.qloc), U, p0, p1, last, static_cast<const long long *>(a.loff), row0,
               reinterpret_cast<long long *>(d_offsets));
        if (!last) {
            long long pass_rows = 0;
            HIP_TRY(hipMemcpyAsync(&pass_rows, a.loff + Cp, 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            row0 += pass_rows;
        }
    }
    return GENIE_OK;
}

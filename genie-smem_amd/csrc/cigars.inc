// cigars.inc -- genie_chain_cigars: the edit script of selected chains of genie_align_chains (included by align.inc, inside
// namespace genie).  The definition is the header's; DESIGN.md section 24 has the reasoning.
//
// The alignment of a chain is cut into pieces: the left extension, the gap fills, the right extension.  A piece with A >= 1 and
// B >= 1 runs through aln_dp<false, true>, which leaves four bits per cell; every other piece is one op in closed form.
//   CG0 lu_check_kernel / chain_check_kernel / align_unit_kernel   as genie_align_chains runs them
//   CG1 cigar_plan_kernel   one lane per selected chain: its index, the walk along its members, the end cells read off d_aln, the
//                           flags 4 and 16, the direction bytes its pieces need
//   CG2 cigar_room_kernel   one block: the running sum of the needs, flag 8 where it passes dir_bytes, the totals
//   CG3 cigar_fill_kernel   one wave per selected chain with room: the pieces through aln_dp with directions, in the order gaps
//                           (from the last member backwards), right extension, left extension
//   CG4 cigar_trace_kernel  one lane per selected chain, twice: it counts the ops (and writes d_info), launch_compact turns the
//                           counts into d_cigar_offsets, and it runs again to write the ops.  The left extension is traced
//                           first and written forwards from the chain's first op, everything else is traced from the right
//                           clip backwards and written backwards from its last op; the two meet at the first member.
namespace {

enum : int { kOpI = 1, kOpD = 2, kOpS = 4, kOpEq = 7, kOpX = 8 };
enum : int { kCgSkipped = 4, kCgNoRoom = 8, kCgBad = 16 };

struct CigarArea {
    int *flag;                            // the verdict of the offset checks
    int32_t *unit;                        // per chain
    int32_t *nops;                        // per selected chain
    long long *need, *diroff;             // per selected chain: direction bytes, and where they begin
    unsigned long long *scan_tmp;         // launch_compact's
    uint8_t *dirs;                        // dir_bytes
};

inline int64_t cigar_layout(uint8_t *base, int64_t cap_chains, int64_t n_sel, int64_t dir_bytes, CigarArea *a)
{
    Carver c{base};
    c.take(a->flag, 8);
    c.take(a->unit, cap_chains * 4);
    c.take(a->nops, n_sel * 4);
    c.take(a->need, n_sel * 8);
    c.take(a->diroff, n_sel * 8);
    c.take(a->scan_tmp, compact_tmp_bytes(n_sel));
    c.take(a->dirs, dir_bytes);
    return c.at;
}

// everything about chain c that its pieces need, as align_kernel derives it
struct CgChain {
    AlnRead rd;
    long long rbase;
    int nrows, lc, clo, chi, last;
};

__device__ __forceinline__ CgChain cg_chain(const DevIndex &ix, const AlignInput &in, const int32_t *__restrict__ unit, long long c)
{
    long long u = unit[c];
    u = u < 0 ? 0 : (u > in.U - 1 ? in.U - 1 : u);
    const long long rd_i = in.S == 2 ? u >> 1 : u;
    const long long ro = in.roff[rd_i];
    CgChain k;
    k.rd = AlnRead{in.bases, ro, (int)(in.roff[rd_i + 1] - ro), in.S == 2 ? (int)(u & 1) : 0};
    k.rbase = in.off[u];
    k.nrows = (int)(in.off[u + 1] - k.rbase);
    k.lc = (int)(c - in.coff[u]);
    const int4 ch = in.chains[2 * c + 1];
    k.clo = 0;
    k.chi = ix.n;
    if (in.ctg) {
        const int g = ch.z < 0 ? 0 : (ch.z > in.nctg - 1 ? in.nctg - 1 : ch.z);
        const long long a = in.ctg[g], b = in.ctg[g + 1];
        k.clo = (int)(a < 0 ? 0 : (a > ix.n ? ix.n : a));
        k.chi = (int)(b < k.clo ? k.clo : (b > ix.n ? ix.n : b));
    }
    k.last = k.nrows > 0 ? (ch.w < 0 ? 0 : (ch.w > k.nrows - 1 ? k.nrows - 1 : ch.w)) : 0;
    return k;
}

// The walk from the last member backwards: (qs, ts) is the start of the member used last.
struct CgWalk {
    int j, qs, ts;
};
struct CgGap {
    int q0, t0, lp, A, B, dlo, dhi;       // the gap behind the member's l' bases, and its band
    bool too_far;                         // |B - A| > max_indel
};

// the next used member and the gap behind it; false: the chain begins at (qs, ts).  j falls strictly: at most nrows steps.
__device__ __forceinline__ bool cg_next(const AlignInput &in, const CgChain &k, const AlignParams &prm, CgWalk &w, CgGap &g)
{
    while (true) {
        const int pj = in.apred[k.rbase + w.j];
        if (pj < 0 || pj >= w.j || in.achain[k.rbase + pj] != k.lc) return false;
        w.j = pj;
        const AlnMember m = aln_member(in.rows[k.rbase + pj], k.rd.L, k.clo, k.chi);
        int lp = m.l;
        lp = w.qs - m.s < lp ? w.qs - m.s : lp;
        lp = w.ts - m.t < lp ? w.ts - m.t : lp;
        if (lp <= 0) continue;
        g.q0 = m.s + lp;
        g.t0 = m.t + lp;
        g.lp = lp;
        g.A = w.qs - g.q0;
        g.B = w.ts - g.t0;
        const int dd = g.B - g.A;
        g.too_far = (dd < 0 ? -dd : dd) > prm.max_indel;
        g.dlo = (dd < 0 ? dd : 0) - prm.band;
        g.dhi = (dd > 0 ? dd : 0) + prm.band;
        w.qs = m.s;
        w.ts = m.t;
        return true;
    }
}

// the direction bytes of a piece: none in closed form, else A rows of ceil(D / 64) * 32 bytes
__device__ __forceinline__ long long cg_bytes(int A, int B, int dlo, int dhi)
{
    if (A <= 0 || B <= 0) return 0;
    const int D = dhi - dlo + 1 < kAlnDiags ? dhi - dlo + 1 : kAlnDiags;
    return (long long)A * ((D + kWave - 1) / kWave) * 32;
}

// The cells the two extensions consumed, read off the chain's d_aln row; ok: both inside their band and rectangle.
struct CgEnds {
    int ri, rj, li, lj;
    bool ok;
};

__device__ __forceinline__ bool cg_end_ok(long long i, long long j, int A, int avail, int w)
{
    avail = avail > 0 ? avail : 0;
    const int B = avail < A + w ? avail : A + w;
    return i >= 0 && i <= A && j >= 0 && j <= B && j - i <= w && i - j <= w && (i > 0 || j == 0);
}

__device__ __forceinline__ CgEnds cg_ends(const int4 a0, const int4 a1, const CgChain &k, int qs, int ts, int qe, int te, int w)
{
    const long long ri = (long long)a0.z - qe, rj = (long long)a1.x - 1 - te;
    const long long li = (long long)qs - a0.y, lj = (long long)ts - ((long long)a0.w - 1);
    CgEnds e;
    e.ok = cg_end_ok(ri, rj, k.rd.L - qe, k.chi - te, w) && cg_end_ok(li, lj, qs, ts - k.clo, w);
    e.ri = e.ok ? (int)ri : 0;
    e.rj = e.ok ? (int)rj : 0;
    e.li = e.ok ? (int)li : 0;
    e.lj = e.ok ? (int)lj : 0;
    return e;
}

struct CigarSel {
    const long long *sel;                 // or null: k itself
    long long n;
};

__global__ void __launch_bounds__(256) cigar_plan_kernel(DevIndex ix, AlignInput in, AlignParams prm, const int32_t *__restrict__ unit,
                                                         const int4 *__restrict__ aln, CigarSel sl, int4 *__restrict__ info,
                                                         long long *__restrict__ need)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= sl.n) return;
    const long long total = in.coff[in.U];
    const long long C = total < in.cap ? total : in.cap;
    const long long c = sl.sel ? sl.sel[k] : k;
    int flags = 0;
    long long bytes = 0;
    if (c < 0 || c >= C) {
        flags = kCgBad;
    } else {
        const CgChain ch = cg_chain(ix, in, unit, c);
        const int4 a0 = aln[2 * c], a1 = aln[2 * c + 1];
        if ((a1.y & 4) || ch.nrows <= 0) {
            flags = kCgSkipped;
        } else {
            const AlnMember top = aln_member(in.rows[ch.rbase + ch.last], ch.rd.L, ch.clo, ch.chi);
            CgWalk w{ch.last, top.s, top.t};
            CgGap g;
            while (cg_next(in, ch, prm, w, g)) {
                if (g.too_far) {
                    flags = kCgSkipped;
                    break;
                }
                bytes += cg_bytes(g.A, g.B, g.dlo, g.dhi);
            }
            if (!flags) {
                const CgEnds e = cg_ends(a0, a1, ch, w.qs, w.ts, top.s + top.l, top.t + top.l, prm.band);
                if (!e.ok) flags = kCgBad;
                bytes += cg_bytes(e.ri, e.rj, -prm.band, prm.band) + cg_bytes(e.li, e.lj, -prm.band, prm.band);
            }
            if (flags) bytes = 0;
        }
    }
    info[2 * k] = make_int4((int)c, flags, 0, 0);
    info[2 * k + 1] = make_int4(0, 0, 0, 0);
    need[k] = bytes;
}

// The running sum of the needs: chain k has room iff the sum through k is at most dir_bytes.  One block.
__global__ void __launch_bounds__(kScanBlock) cigar_room_kernel(const long long *__restrict__ need, long long n, long long dir_bytes,
                                                                long long *__restrict__ diroff, int4 *__restrict__ info,
                                                                long long *__restrict__ dir_need, long long *__restrict__ totals)
{
    __shared__ unsigned long long wtot[kScanBlock / kWave], wflag[kScanBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    unsigned long long carry = 0, flagged = 0;
    for (long long base = 0; base < n; base += kScanBlock) {
        const long long k = base + threadIdx.x;
        const unsigned long long v = k < n ? (unsigned long long)need[k] : 0ull;
        const unsigned long long inc = wave_inclusive_scan64(v, lane);
        __syncthreads();                                             // the round before has read wtot
        if (lane == kWave - 1) wtot[wave] = inc;
        __syncthreads();
        unsigned long long before = carry;
        for (int w = 0; w < kScanBlock / kWave; w++) {
            const unsigned long long t = wtot[w];
            before += w < wave ? t : 0ull;
            carry += t;
        }
        if (k < n) {
            int4 r = info[2 * k];
            if (before + inc > (unsigned long long)dir_bytes) {
                r.y |= kCgNoRoom;
                info[2 * k] = r;
            }
            flagged += r.y != 0;
            diroff[k] = (long long)(before + inc - v);
            if (dir_need) dir_need[k] = (long long)v;
        }
    }
    flagged = wave_sum64(flagged);
    if (lane == 0) wflag[wave] = flagged;
    __syncthreads();
    if (threadIdx.x == 0 && totals) {
        unsigned long long all = 0;
        for (int w = 0; w < kScanBlock / kWave; w++) all += wflag[w];
        totals[0] = n - (long long)all;
        totals[1] = (long long)all;
        totals[2] = (long long)carry;
    }
}

__global__ void __launch_bounds__(kAlnWaves *kWave) cigar_fill_kernel(DevIndex ix, AlignInput in, AlignParams prm,
                                                                       const int32_t *__restrict__ unit, const int4 *__restrict__ aln,
                                                                       long long n, const int4 *__restrict__ info,
                                                                       const long long *__restrict__ need,
                                                                       const long long *__restrict__ diroff, uint8_t *__restrict__ dirs)
{
    __shared__ int2 rows_lds[kAlnWaves][kAlnDiags];
    __shared__ __attribute__((aligned(16))) uint8_t ref_lds[kAlnWaves][kAlnRefBytes];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int2 *st = rows_lds[wave];
    uint8_t *rw = ref_lds[wave];
    for (long long k = (long long)blockIdx.x * kAlnWaves + wave; k < n; k += (long long)gridDim.x * kAlnWaves) {
        const int4 head = info[2 * k];
        if (head.y != 0 || need[k] <= 0) continue;                   // flagged, or closed forms alone
        const long long c = head.x;
        const CgChain ch = cg_chain(ix, in, unit, c);
        const AlnMember top = aln_member(in.rows[ch.rbase + ch.last], ch.rd.L, ch.clo, ch.chi);
        uint8_t *at = dirs + diroff[k];
        CgWalk w{ch.last, top.s, top.t};
        CgGap g;
        while (cg_next(in, ch, prm, w, g)) {
            if (g.A > 0 && g.B > 0) aln_dp<false, true>(ix, ch.rd, g.q0, g.t0, 1, g.A, g.B, g.dlo, g.dhi, prm, lane, st, rw, at);
            at += cg_bytes(g.A, g.B, g.dlo, g.dhi);
        }
        const int qe = top.s + top.l, te = top.t + top.l;
        const CgEnds e = cg_ends(aln[2 * c], aln[2 * c + 1], ch, w.qs, w.ts, qe, te, prm.band);
        if (e.ri > 0 && e.rj > 0) aln_dp<false, true>(ix, ch.rd, qe, te, 1, e.ri, e.rj, -prm.band, prm.band, prm, lane, st, rw, at);
        at += cg_bytes(e.ri, e.rj, -prm.band, prm.band);
        if (e.li > 0 && e.lj > 0)
            aln_dp<false, true>(ix, ch.rd, w.qs - 1, w.ts - 1, -1, e.li, e.lj, -prm.band, prm.band, prm, lane, st, rw, at);
    }
}

// Ops as they are found, neighbouring equal ops merged, written to out[pos] and on in direction step while lo <= pos < hi.
struct CgOps {
    uint32_t *out;
    long long lo, hi, pos;
    int step, op, n;
    long long len;                        // the op that is still open
    int n_eq, n_x, n_ins, n_del;

    __device__ __forceinline__ void flush()
    {
        if (len > 0) {
            if (out && pos >= lo && pos < hi) out[pos] = ((uint32_t)len << 4) | (uint32_t)op;
            pos += step;
            n++;
        }
        len = 0;
    }
    __device__ __forceinline__ void emit(int o, long long l)
    {
        if (l <= 0) return;
        n_eq += o == kOpEq ? (int)l : 0;
        n_x += o == kOpX ? (int)l : 0;
        n_ins += o == kOpI ? (int)l : 0;
        n_del += o == kOpD ? (int)l : 0;
        if (o == op && len > 0) {
            len += l;
        } else {
            flush();
            op = o;
            len = l;
        }
    }
};

// The canonical path of a piece from (A, B) back to (0, 0): one step per base, at most A + B of them whatever dirs holds.
__device__ __forceinline__ void cg_trace(const uint8_t *__restrict__ dirs, int A, int B, int dlo, int dhi, CgOps &o)
{
    if (A <= 0 || B <= 0) {
        o.emit(A > 0 ? kOpI : kOpD, (long long)(A > 0 ? A : 0) + (B > 0 ? B : 0));
        return;
    }
    const int D = dhi - dlo + 1 < kAlnDiags ? dhi - dlo + 1 : kAlnDiags;
    const long long rowb = ((D + kWave - 1) / kWave) * 32;
    int i = A, j = B, state = 0;                                     // 0: H, 1: F, 2: E
    while (i > 0 || j > 0) {                                         // i + j falls with every step
        if (i == 0 || j == 0) {                                      // the border: one gap to (0, 0)
            o.emit(i > 0 ? kOpI : kOpD, i + j);
            break;
        }
        const int idx = j - i - dlo;
        if (idx < 0 || idx >= D) break;                              // no path from a finite cell leaves the band
        const int nib = (dirs[(long long)(i - 1) * rowb + (idx >> 1)] >> ((idx & 1) * 4)) & 15;
        if (state == 0) {
            const int src = nib & 3;
            if (src <= 1) {
                o.emit(src ? kOpX : kOpEq, 1);
                i--;
                j--;
                continue;
            }
            state = src == 2 ? 1 : 2;
        }
        if (state == 1) {
            o.emit(kOpI, 1);
            state = (nib & 4) ? 1 : 0;
            i--;
        } else {
            o.emit(kOpD, 1);
            state = (nib & 8) ? 2 : 0;
            j--;
        }
    }
}

// offsets == null: the counting run, which writes nops and the rest of d_info; else the writing run.
__global__ void __launch_bounds__(256) cigar_trace_kernel(DevIndex ix, AlignInput in, AlignParams prm, const int32_t *__restrict__ unit,
                                                          const int4 *__restrict__ aln, long long n, int4 *__restrict__ info,
                                                          const long long *__restrict__ diroff, const uint8_t *__restrict__ dirs,
                                                          int32_t *__restrict__ nops, const long long *__restrict__ offsets,
                                                          uint32_t *__restrict__ cigar, long long cap_ops)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int4 head = info[2 * k];
    if (head.y != 0) {
        if (!offsets) nops[k] = 0;
        return;
    }
    const long long c = head.x;
    const CgChain ch = cg_chain(ix, in, unit, c);
    const AlnMember top = aln_member(in.rows[ch.rbase + ch.last], ch.rd.L, ch.clo, ch.chi);
    const int qe = top.s + top.l, te = top.t + top.l, bw = prm.band;
    CgWalk w{ch.last, top.s, top.t};
    CgGap g;
    long long gap_bytes = 0;
    while (cg_next(in, ch, prm, w, g)) gap_bytes += cg_bytes(g.A, g.B, g.dlo, g.dhi);
    const int4 a0 = aln[2 * c];
    const CgEnds e = cg_ends(a0, aln[2 * c + 1], ch, w.qs, w.ts, qe, te, bw);
    const uint8_t *base = dirs + diroff[k];
    const long long first = offsets ? offsets[k] : 0, count = offsets ? nops[k] : 0;
    const long long hi = first + count < cap_ops ? first + count : cap_ops;
    CgOps fwd{offsets ? cigar : nullptr, first, hi, first, 1, 0, 0, 0, 0, 0, 0, 0};
    CgOps bwd{offsets ? cigar : nullptr, first, hi, first + count - 1, -1, 0, 0, 0, 0, 0, 0, 0};
    // forwards: the left clip and the left extension, whose program runs on the reversed strings
    fwd.emit(kOpS, a0.y);
    cg_trace(base + gap_bytes + cg_bytes(e.ri, e.rj, -bw, bw), e.li, e.lj, -bw, bw, fwd);
    // backwards: the right clip, the right extension, the last member, and gap and member in turn down to the first
    bwd.emit(kOpS, ch.rd.L - (qe + e.ri));
    cg_trace(base + gap_bytes, e.ri, e.rj, -bw, bw, bwd);
    bwd.emit(kOpEq, top.l);
    w = CgWalk{ch.last, top.s, top.t};
    const uint8_t *at = base;
    while (cg_next(in, ch, prm, w, g)) {
        cg_trace(at, g.A, g.B, g.dlo, g.dhi, bwd);
        at += cg_bytes(g.A, g.B, g.dlo, g.dhi);
        bwd.emit(kOpEq, g.lp);
    }
    // the two meet: one op if they end alike
    if (fwd.len > 0 && bwd.len > 0 && fwd.op == bwd.op) {
        fwd.len += bwd.len;
        bwd.len = 0;
    }
    fwd.flush();
    bwd.flush();
    if (!offsets) {
        const int n_x = fwd.n_x + bwd.n_x, n_ins = fwd.n_ins + bwd.n_ins, n_del = fwd.n_del + bwd.n_del;
        nops[k] = fwd.n + bwd.n;
        info[2 * k] = make_int4(head.x, 0, fwd.n + bwd.n, n_x + n_ins + n_del);
        info[2 * k + 1] = make_int4(fwd.n_eq + bwd.n_eq, n_x, n_ins, n_del);
    }
}

}  // namespace

int64_t chain_cigars_workspace_bytes(int64_t U, int64_t cap_chains, int64_t n_sel, int64_t dir_bytes)
{
    (void)U;                                                         // nothing is kept per unit
    CigarArea a;
    return cigar_layout(nullptr, cap_chains, n_sel, dir_bytes, &a);
}

int launch_chain_cigars(const genie_index *ix, const ContigTable &ctg, const CsrBatch &b, const AlignBatch &ab, const AlignParams &prm,
                        const int32_t *d_aln, const CigarOut &out, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t U = ab.U, cap = ab.cap_chains;
    CigarArea a;
    cigar_layout(static_cast<uint8_t *>(b.ws), cap, out.sel ? out.n_sel : cap, out.dir_bytes, &a);
    const long long *roff = reinterpret_cast<const long long *>(b.read_offsets);
    const long long *off = reinterpret_cast<const long long *>(ab.offsets);
    const long long *coff = reinterpret_cast<const long long *>(ab.chain_offsets);
    long long n = out.sel ? out.n_sel : 0;
    if (U > 0) {
        HIP_TRY(hipMemsetAsync(a.flag, 0, 8, s));
        LAUNCH_BLOCKS(lu_check_kernel, (b.N + 1 + 255) / 256, 256, 0, s, roff, (long long)b.N, (long long)b.total_bases,
                      (long long)b.max_len, (int)GENIE_MODE_BWA, 0, b.strands(), a.flag, static_cast<int32_t *>(nullptr),
                      static_cast<long long *>(nullptr), static_cast<long long *>(nullptr));
        LAUNCH_BLOCKS(chain_check_kernel, (U + 1 + 255) / 256, 256, 0, s, off, (long long)U, (long long)ab.total_rows, a.flag);
        int bad = 0;
        long long total = 0;
        HIP_TRY(hipMemcpyAsync(&bad, a.flag, 4, hipMemcpyDeviceToHost, s));
        if (!out.sel) HIP_TRY(hipMemcpyAsync(&total, coff + U, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (bad) return GENIE_E_INVALID;
        if (!out.sel) n = total < 0 ? 0 : (total < cap ? total : cap);
    }
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(out.offsets, 0, 8, s));
        if (out.totals) HIP_TRY(hipMemsetAsync(out.totals, 0, 24, s));
        return GENIE_OK;
    }
    if (cap > 0 && U > 0) LAUNCH_BLOCKS(align_unit_kernel, (cap + 255) / 256, 256, 0, s, coff, (long long)U, (long long)cap, a.unit);
    // U == 0: no chain exists, the plan flags every index and nothing below reads the batch
    const AlignInput in{b.bases, roff, b.strands(), off, reinterpret_cast<const int4 *>(ab.rows), ab.anchor_chain, ab.anchor_pred, coff,
                        reinterpret_cast<const int4 *>(ab.chains), (long long)U, U > 0 ? (long long)cap : 0ll,
                        ctg.n_contigs > 0 ? reinterpret_cast<const long long *>(ctg.offsets) : nullptr, (int)ctg.n_contigs};
    const int32_t *unit = a.unit;
    const int4 *aln = reinterpret_cast<const int4 *>(d_aln);
    int4 *info = reinterpret_cast<int4 *>(out.info);
    const CigarSel sl{reinterpret_cast<const long long *>(out.sel), n};
    LAUNCH_BLOCKS(cigar_plan_kernel, (n + 255) / 256, 256, 0, s, ix->dev, in, prm, unit, aln, sl, info, a.need);
    LAUNCH(cigar_room_kernel, dim3(1), dim3(kScanBlock), 0, s, static_cast<const long long *>(a.need), n, (long long)out.dir_bytes,
           a.diroff, info, reinterpret_cast<long long *>(out.dir_need), reinterpret_cast<long long *>(out.totals));
    const long long want = (n + kAlnWaves - 1) / kAlnWaves, most = (long long)(ix->num_cus > 0 ? ix->num_cus : 256) * 4;
    LAUNCH(cigar_fill_kernel, dim3((unsigned)std::min(want, most)), dim3(kAlnWaves * kWave), 0, s, ix->dev, in, prm, unit, aln, n,
           static_cast<const int4 *>(info), static_cast<const long long *>(a.need), static_cast<const long long *>(a.diroff), a.dirs);
    LAUNCH_BLOCKS(cigar_trace_kernel, (n + 255) / 256, 256, 0, s, ix->dev, in, prm, unit, aln, n, info,
                  static_cast<const long long *>(a.diroff), static_cast<const uint8_t *>(a.dirs), a.nops,
                  static_cast<const long long *>(nullptr), static_cast<uint32_t *>(nullptr), 0ll);
    if (int rc = launch_compact(a.nops, nullptr, n, 0x7FFFFFFF, out.offsets, nullptr, 0, a.scan_tmp, stream)) return rc;
    if (out.cigar && out.cap_ops > 0)
        LAUNCH_BLOCKS(cigar_trace_kernel, (n + 255) / 256, 256, 0, s, ix->dev, in, prm, unit, aln, n, info,
                      static_cast<const long long *>(a.diroff), static_cast<const uint8_t *>(a.dirs), a.nops,
                      reinterpret_cast<const long long *>(out.offsets), out.cigar, (long long)out.cap_ops);
    return GENIE_OK;
}

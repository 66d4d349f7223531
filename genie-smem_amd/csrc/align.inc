// align.inc -- genie_align_chains: every chain of genie_chain_mems aligned -- a banded affine gap fill between its members and a
// banded extension at both ends -- score and end points only (included by kernels.hip behind chains.inc, inside namespace
// genie).  The definition is the header's; DESIGN.md section 23 has the reasoning.
//
// One wave owns a chain from its first load to its one store; chains are taken grid-stride, four waves to a block.  Everything
// about the chain (its unit, its members, the trimming) is wave-uniform: every lane computes it from the same loads.
//   AL0 lu_check_kernel / chain_check_kernel   the read offsets and the row offsets, as their producing calls check them; the
//                             host reads the flag: the call's one synchronisation
//   AL1 align_unit_kernel     one lane per chain: its unit, by a bisection of d_chain_offsets (clamped: any table terminates)
//   AL2 align_kernel          per chain: the walk from `last` along d_anchor_pred, the trimming, a dynamic program per gap and
//                             per end
//   AL3 align_totals_kernel   {chains aligned, chains skipped}: a sum over the flags, by one block
// The dynamic program (aln_dp): LANES OVER DIAGONALS, ROWS OVER QUERY BASES.  Lane k of chunk c holds diagonal d = dlo + 64 c + k
// of the band; row i is query base i.  Cell (i, j = i + d):
//   diagonal  H(i-1, j-1) is the lane's own diagonal in the row before
//   vertical  (a gap that consumes query) comes from diagonal d + 1 of the row before: the next lane
//   horizontal (a gap that consumes reference) runs along the row: with x_k = max(diagonal, vertical)(i, k) + k e it is
//             max_{k < j} x_k - o - j e, an exclusive wave max-scan; a carry takes the maximum from chunk to chunk
// The row before, (H, vertical) per diagonal, lives in the wave's LDS: 8 bytes per diagonal, 8 KB at 1024 diagonals.  A chunk
// reads (d, d + 1) and then writes d, chunks ascending, so one copy of the row is enough.  Per 64 rows the wave stages its
// query bases (one per lane, handed out by v_readlane) and the window of the reference the rows can touch: 64-bit words of the
// packed reference, one per lane, unpacked to one byte per base in LDS.  Chunks without a cell inside the rectangle are not run.
// -infinity is kAlnNeg = -2^30: the host has checked that no path's score reaches it, every cell of the band inside the
// rectangle is reachable, and a value that falls below kAlnNeg is set back to it.
namespace {

constexpr int kAlnWaves = 4;                                  // waves per block
constexpr int kAlnDiags = GENIE_ALIGN_MAX_DIAGS;              // diagonals of the widest band
constexpr int kAlnRows = kWave;                               // rows per staging
constexpr int kAlnRefWords = (kAlnRows + kAlnDiags + 62) / 32 + 1;      // 32-base words a staging can touch: 36
constexpr int kAlnRefBytes = kAlnRefWords * 32;
constexpr int kAlnNeg = -(1 << 30);
static_assert(kAlnDiags == 1024 && kAlnRefWords <= kWave, "one word per lane");
static_assert(4 * kAlnWaves * (kAlnDiags * 8 + kAlnRefBytes) <= 160 * 1024, "four blocks per CU");

struct AlignArea {
    int *flag;                            // AL0's verdict
    int32_t *unit;                        // per chain
};

inline int64_t align_layout(uint8_t *base, int64_t cap_chains, AlignArea *a)
{
    Carver c{base};
    c.take(a->flag, 8);
    c.take(a->unit, cap_chains * 4);
    return c.at;
}

// a strand-read: position p of strand `rev` of the read at bases[o .. o + L)
struct AlnRead {
    const uint8_t *bases;
    long long o;
    int L, rev;
};

__device__ __forceinline__ uint32_t aln_query(const AlnRead &r, int p)
{
    p = p < 0 ? 0 : (p > r.L - 1 ? r.L - 1 : p);
    const uint32_t c = r.bases[r.o + (r.rev ? r.L - 1 - p : p)];
    return (r.rev && c <= 3u) ? 3u - c : c;
}

__device__ __forceinline__ int aln_wave_max(int v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o, kWave);
        v = w > v ? w : v;
    }
    return v;
}

__device__ __forceinline__ int aln_wave_min(int v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const int w = __shfl_xor(v, o, kWave);
        v = w < v ? w : v;
    }
    return v;
}

// the lanes of a wave run in step; this keeps the compiler from moving an LDS access of one lane across that of another
__device__ __forceinline__ void aln_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// four bases (the byte v, first base in its top bits) as four bytes, first base lowest
__device__ __forceinline__ uint32_t aln_spread(uint32_t v)
{
    return ((v >> 6) & 3u) | (((v >> 4) & 3u) << 8) | (((v >> 2) & 3u) << 16) | ((v & 3u) << 24);
}

struct AlnEnd {
    int value, qi, rj, to_end;            // gap fill: value = H(A, B) alone
};

// The banded affine program on x[0 .. A), y[0 .. B) over the diagonals [dlo, dhi], dlo <= 0 <= dhi, at most kAlnDiags of them:
// x_i is position q0 + dir i of the strand-read, y_j base t0 + dir j of the reference.  kExt: the extension's rule, else
// H(A, B).  A >= 1.  st: the wave's row, kAlnDiags (H, vertical); rw: its kAlnRefBytes reference bases.
// kTrace (cigars.inc): every cell of the rows 1 .. min(A, B - dlo) also leaves four bits in dirs, where it came from: bits 0-1 the
// source of H, taken in the canonical order (0 the diagonal on a match, 1 the diagonal otherwise, 2 F, 3 E), bit 2: F(i, j) is
// F(i-1, j) - e, bit 3: E(i, j) is E(i, j-1) - e.  Row i is ceil(D / 64) * 32 bytes, two diagonals to a byte, the even one low.
template <bool kExt, bool kTrace = false>
__device__ __forceinline__ AlnEnd aln_dp(const DevIndex &ix, const AlnRead &rd, int q0, int t0, int dir, int A, int B, int dlo, int dhi,
                                         const AlignParams &p, int lane, int2 *__restrict__ st, uint8_t *__restrict__ rw,
                                         uint8_t *__restrict__ dirs = nullptr)
{
    const int D = dhi - dlo + 1 < kAlnDiags ? dhi - dlo + 1 : kAlnDiags;
    const int nchunks = (D + kWave - 1) / kWave;
    const int oe = p.gap_open + p.gap_extend, e = p.gap_extend;
    const int last_word = (ix.n - 1) >> 5;
    for (int c = 0; c < nchunks; c++) {                              // row 0: a gap from (0, 0) along the reference
        const int idx = c * kWave + lane, d = dlo + idx;
        if (idx < D) st[idx] = make_int2(d == 0 ? 0 : (d > 0 && d <= B ? -p.gap_open - d * e : kAlnNeg), kAlnNeg);
    }
    const int last = A < B - dlo ? A : B - dlo;                      // the rows that have a cell inside the rectangle
    int bh = 0, bs = 0, bi = 0;                                      // the lane's best cell: (H, i + j, i); (0, 0) to begin with
    int gh = kAlnNeg, gj = 0x7fffffff;                               // row A: (H, j)
    for (int i0 = 0; i0 < last; i0 += kAlnRows) {
        const int cnt = last - i0 < kAlnRows ? last - i0 : kAlnRows;
        const uint32_t xq = i0 + lane < A ? aln_query(rd, q0 + dir * (i0 + lane)) : 4u;
        // the reference the rows i0 + 1 .. i0 + cnt touch: y_j, j from jmin to jmax
        const int jmin = i0 + dlo > 0 ? i0 + dlo : 0, jmax = i0 + cnt + dhi - 1 < B - 1 ? i0 + cnt + dhi - 1 : B - 1;
        int w0 = 0;
        aln_wave_sync();                                             // the rows before have read their window
        if (jmin <= jmax) {
            const int ta = t0 + dir * jmin, tb = t0 + dir * jmax;
            w0 = (ta < tb ? ta : tb) >> 5;
            int nw = ((ta < tb ? tb : ta) >> 5) - w0 + 1;
            nw = nw < kAlnRefWords ? nw : kAlnRefWords;
            if (lane < nw) {
                int wi = w0 + lane;
                wi = wi < 0 ? 0 : (wi > last_word ? last_word : wi);
                const uint64_t w = reinterpret_cast<const uint64_t *>(ix.ref)[(long long)wi * 2];
                const uint32_t hi = (uint32_t)(w >> 32), lo = (uint32_t)w;
                uint4 *dst = reinterpret_cast<uint4 *>(rw + 32 * lane);
                dst[0] = make_uint4(aln_spread(hi >> 24), aln_spread((hi >> 16) & 255u), aln_spread((hi >> 8) & 255u), aln_spread(hi & 255u));
                dst[1] = make_uint4(aln_spread(lo >> 24), aln_spread((lo >> 16) & 255u), aln_spread((lo >> 8) & 255u), aln_spread(lo & 255u));
            }
        }
        aln_wave_sync();
        for (int k = 0; k < cnt; k++) {
            const int i = i0 + 1 + k;
            const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)xq, k);
            const int first_idx = -i - dlo > 0 ? -i - dlo : 0, last_idx = D - 1 < B - i - dlo ? D - 1 : B - i - dlo;
            int carry = kAlnNeg;                                     // the largest x_k of the chunks before
            [[maybe_unused]] int ecarry = kAlnNeg;                   // kTrace: E of the last lane of the chunk before
            for (int c = first_idx / kWave; c <= last_idx / kWave; c++) {
                const int idx = c * kWave + lane, d = dlo + idx, j = i + d;
                const bool inb = idx < D, valid = inb && j >= 0 && j <= B;
                aln_wave_sync();                                     // the row before is written
                const int2 me = st[idx < kAlnDiags ? idx : kAlnDiags - 1];
                const int2 up = idx + 1 < D ? st[idx + 1] : make_int2(kAlnNeg, kAlnNeg);
                aln_wave_sync();                                     // ... and read before this row overwrites it
                uint32_t y = 4u;
                if (valid && j >= 1) {
                    int li = t0 + dir * (j - 1) - 32 * w0;
                    li = li < 0 ? 0 : (li > kAlnRefBytes - 1 ? kAlnRefBytes - 1 : li);
                    y = rw[li];
                }
                const int sc = (x == y && x <= 3u) ? p.match : -p.mismatch;
                const int diag = (j >= 1 && me.x > kAlnNeg) ? me.x + sc : kAlnNeg;
                int v = up.x - oe > up.y - e ? up.x - oe : up.y - e;
                v = v > kAlnNeg ? v : kAlnNeg;
                const int hp = diag > v ? diag : v;
                int incl = valid ? hp + j * e : kAlnNeg;
#pragma unroll
                for (int o = 1; o < kWave; o <<= 1) {
                    const int t = __shfl_up(incl, o, kWave);
                    if (lane >= o) incl = t > incl ? t : incl;
                }
                int pm = __shfl_up(incl, 1, kWave);
                pm = (lane == 0 || pm < carry) ? carry : pm;
                int g = pm - p.gap_open - j * e;
                g = g > kAlnNeg ? g : kAlnNeg;
                int h = hp > g ? hp : g;
                if (!valid) {
                    h = kAlnNeg;
                    v = kAlnNeg;
                }
                if (inb) st[idx] = make_int2(h, v);
                if constexpr (kTrace) {
                    int ep = __shfl_up(g, 1, kWave);                 // E(i, j - 1)
                    ep = lane == 0 ? ecarry : ep;
                    ecarry = __builtin_amdgcn_readlane(g, kWave - 1);
                    const int src = (j >= 1 && h == diag) ? ((x == y && x <= 3u) ? 0 : 1) : (h == v ? 2 : 3);
                    const int nib = src | (up.x - oe > up.y - e ? 0 : 4) | (g == ep - e ? 8 : 0);
                    const int odd = __shfl_down(nib, 1, kWave);
                    if (!(lane & 1)) dirs[(long long)(i - 1) * (nchunks * 32) + c * 32 + (lane >> 1)] = (uint8_t)(nib | (odd << 4));
                }
                const int top = __builtin_amdgcn_readlane(incl, kWave - 1);
                carry = top > carry ? top : carry;
                if (kExt) {
                    const int s = i + j;
                    if (valid && (h > bh || (h == bh && (s < bs || (s == bs && i < bi))))) {
                        bh = h;
                        bs = s;
                        bi = i;
                    }
                }
                if (valid && i == A && (kExt ? (h > gh || (h == gh && j < gj)) : j == B)) {
                    gh = h;
                    gj = j;
                }
            }
        }
    }
    aln_wave_sync();
    AlnEnd r{0, 0, 0, 0};
    const int G = aln_wave_max(gh);
    if (!kExt) {
        r.value = G;
        return r;
    }
    const int M = aln_wave_max(bh);
    const int sm = aln_wave_min(bh == M ? bs : 0x7fffffff);
    const int im = aln_wave_min(bh == M && bs == sm ? bi : 0x7fffffff);
    if (last == A && G + p.end_bonus >= M) {                         // row A has a cell: a tie goes to the end
        r.value = G + p.end_bonus;
        r.qi = A;
        r.rj = aln_wave_min(gh == G ? gj : 0x7fffffff);
        r.to_end = 1;
    } else {
        r.value = M;
        r.qi = im;
        r.rj = sm - im;
    }
    return r;
}

// x[0 .. A) of the strand-read from q0 on, in direction dir, extended along the `avail` reference bases from t0 on
__device__ __forceinline__ AlnEnd aln_extend(const DevIndex &ix, const AlnRead &rd, int q0, int t0, int dir, int A, int avail,
                                             const AlignParams &p, int lane, int2 *__restrict__ st, uint8_t *__restrict__ rw)
{
    if (A <= 0) return AlnEnd{p.end_bonus, 0, 0, 1};
    avail = avail > 0 ? avail : 0;
    const int B = avail < A + p.band ? avail : A + p.band;
    return aln_dp<true>(ix, rd, q0, t0, dir, A, B, -p.band, p.band, p, lane, st, rw);
}

struct AlnMember {
    int s, l, t;
};

// row (start, end, pos, .) with its positions clamped to [0, L] and [clo, chi)
__device__ __forceinline__ AlnMember aln_member(const int4 r, int L, int clo, int chi)
{
    AlnMember m;
    m.s = r.x < 0 ? 0 : (r.x > L ? L : r.x);
    const int e = r.y < m.s ? m.s : (r.y > L ? L : r.y);
    const int t = (int)((unsigned)r.z - 1u);
    const int thi = chi > clo ? chi - 1 : clo;
    m.t = t < clo ? clo : (t > thi ? thi : t);
    const int room = chi - m.t > 0 ? chi - m.t : 0;
    m.l = e - m.s < room ? e - m.s : room;
    return m;
}

struct AlignInput {
    const uint8_t *bases;
    const long long *roff;
    int S;
    const long long *off;
    const int4 *rows;
    const int32_t *achain, *apred;
    const long long *coff;
    const int4 *chains;
    long long U, cap;
    const long long *ctg;                 // or null
    int nctg;
};

__global__ void __launch_bounds__(256) align_unit_kernel(const long long *__restrict__ coff, long long U, long long cap,
                                                         int32_t *__restrict__ unit)
{
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long C = coff[U] < cap ? coff[U] : cap;
    if (c >= C) return;
    long long lo = 0, hi = U;                                        // the last u in [0, U) with coff[u] <= c
    while (lo < hi - 1) {
        const long long mid = (lo + hi) >> 1;
        if (coff[mid] <= c) lo = mid; else hi = mid;
    }
    unit[c] = (int32_t)lo;
}

__global__ void __launch_bounds__(kAlnWaves *kWave) align_kernel(DevIndex ix, AlignInput in, AlignParams prm,
                                                                  const int32_t *__restrict__ unit, int4 *__restrict__ aln)
{
    __shared__ int2 rows_lds[kAlnWaves][kAlnDiags];
    __shared__ __attribute__((aligned(16))) uint8_t ref_lds[kAlnWaves][kAlnRefBytes];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int2 *st = rows_lds[wave];
    uint8_t *rw = ref_lds[wave];
    const long long total = in.coff[in.U];
    const long long C = total < in.cap ? total : in.cap;
    for (long long c = (long long)blockIdx.x * kAlnWaves + wave; c < C; c += (long long)gridDim.x * kAlnWaves) {
        long long u = unit[c];
        u = u < 0 ? 0 : (u > in.U - 1 ? in.U - 1 : u);
        const long long rd_i = in.S == 2 ? u >> 1 : u;
        const long long ro = in.roff[rd_i];
        const AlnRead rd{in.bases, ro, (int)(in.roff[rd_i + 1] - ro), in.S == 2 ? (int)(u & 1) : 0};
        const int L = rd.L;
        const long long rbase = in.off[u];
        const int nrows = (int)(in.off[u + 1] - rbase);
        const int lc = (int)(c - in.coff[u]);
        const int4 ch = in.chains[2 * c + 1];
        int clo = 0, chi = ix.n;
        if (in.ctg) {
            const int g = ch.z < 0 ? 0 : (ch.z > in.nctg - 1 ? in.nctg - 1 : ch.z);
            const long long a = in.ctg[g], b = in.ctg[g + 1];
            clo = (int)(a < 0 ? 0 : (a > ix.n ? ix.n : a));
            chi = (int)(b < clo ? clo : (b > ix.n ? ix.n : b));
        }
        int4 out0 = make_int4(0, 0, 0, 0), out1 = make_int4(0, 4, 0, 0);        // skipped until aligned
        if (nrows > 0) {
            int j = ch.w < 0 ? 0 : (ch.w > nrows - 1 ? nrows - 1 : ch.w);
            const AlnMember top = aln_member(in.rows[rbase + j], L, clo, chi);
            int qs = top.s, ts = top.t;
            int score = prm.match * top.l, matched = top.l, used = 1;
            bool skip = false;
            while (true) {
                const int pj = in.apred[rbase + j];
                if (pj < 0 || pj >= j || in.achain[rbase + pj] != lc) break;
                j = pj;                                              // falls strictly: at most nrows steps
                const AlnMember m = aln_member(in.rows[rbase + j], L, clo, chi);
                int lp = m.l;
                lp = qs - m.s < lp ? qs - m.s : lp;
                lp = ts - m.t < lp ? ts - m.t : lp;
                if (lp <= 0) continue;
                const int A = qs - (m.s + lp), B = ts - (m.t + lp), dd = B - A;
                if ((dd < 0 ? -dd : dd) > prm.max_indel) {
                    skip = true;
                    break;
                }
                int fill;
                if (A == 0 || B == 0)                                // one gap, or nothing: H(A, B) in closed form
                    fill = A + B == 0 ? 0 : -prm.gap_open - (A + B) * prm.gap_extend;
                else
                    fill = aln_dp<false>(ix, rd, m.s + lp, m.t + lp, 1, A, B, (dd < 0 ? dd : 0) - prm.band, (dd > 0 ? dd : 0) + prm.band,
                                         prm, lane, st, rw).value;
                score += prm.match * lp + fill;
                matched += lp;
                used++;
                qs = m.s;
                ts = m.t;
            }
            if (!skip) {
                const int qe = top.s + top.l, te = top.t + top.l;
                const AlnEnd right = aln_extend(ix, rd, qe, te, 1, L - qe, chi - te, prm, lane, st, rw);
                const AlnEnd left = aln_extend(ix, rd, qs - 1, ts - 1, -1, qs, ts - clo, prm, lane, st, rw);
                out0 = make_int4(score + right.value + left.value, qs - left.qi, qe + right.qi, ts - left.rj + 1);
                out1 = make_int4(te + right.rj + 1, left.to_end | (right.to_end << 1), used, matched);
            }
        }
        if (lane == 0) {
            aln[2 * c] = out0;
            aln[2 * c + 1] = out1;
        }
    }
}

// {chains aligned, chains skipped}, by one block
__global__ void __launch_bounds__(kScanBlock) align_totals_kernel(const long long *__restrict__ coff, long long U, long long cap,
                                                                  const int4 *__restrict__ aln, long long *__restrict__ totals)
{
    __shared__ unsigned long long wsum[kScanBlock / kWave];
    const long long C = coff[U] < cap ? coff[U] : cap;
    unsigned long long d = 0;
    for (long long c = threadIdx.x; c < C; c += kScanBlock) d += (unsigned long long)((aln[2 * c + 1].y >> 2) & 1);
    d = wave_sum64(d);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int w = 0; w < kScanBlock / kWave; w++) all += wsum[w];
        totals[0] = (C > 0 ? C : 0) - (long long)all;
        totals[1] = (long long)all;
    }
}

}  // namespace

#include "cigars.inc"
#include "select.inc"
#include "pairs.inc"
#include "insert_size.inc"

int64_t align_chains_workspace_bytes(int64_t U, int64_t cap_chains)
{
    (void)U;                                                         // nothing is kept per unit
    AlignArea a;
    return align_layout(nullptr, cap_chains, &a);
}

int launch_align_chains(const genie_index *ix, const ContigTable &ctg, const CsrBatch &b, const AlignBatch &ab, const AlignParams &prm,
                        int32_t *d_aln, int64_t *d_totals, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t U = ab.U;
    if (U == 0) {
        if (d_totals) HIP_TRY(hipMemsetAsync(d_totals, 0, 16, s));
        return GENIE_OK;
    }
    AlignArea a;
    align_layout(static_cast<uint8_t *>(b.ws), ab.cap_chains, &a);
    const long long *roff = reinterpret_cast<const long long *>(b.read_offsets);
    const long long *off = reinterpret_cast<const long long *>(ab.offsets);
    const long long *coff = reinterpret_cast<const long long *>(ab.chain_offsets);
    HIP_TRY(hipMemsetAsync(a.flag, 0, 8, s));
    LAUNCH_BLOCKS(lu_check_kernel, (b.N + 1 + 255) / 256, 256, 0, s, roff, (long long)b.N, (long long)b.total_bases, (long long)b.max_len,
                  (int)GENIE_MODE_BWA, 0, b.strands(), a.flag, static_cast<int32_t *>(nullptr), static_cast<long long *>(nullptr),
                  static_cast<long long *>(nullptr));
    LAUNCH_BLOCKS(chain_check_kernel, (U + 1 + 255) / 256, 256, 0, s, off, (long long)U, (long long)ab.total_rows, a.flag);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, a.flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return GENIE_E_INVALID;
    const long long cap = ab.cap_chains;
    if (cap == 0) {
        if (d_totals) HIP_TRY(hipMemsetAsync(d_totals, 0, 16, s));
        return GENIE_OK;
    }
    LAUNCH_BLOCKS(align_unit_kernel, (cap + 255) / 256, 256, 0, s, coff, (long long)U, cap, a.unit);
    const AlignInput in{b.bases, roff, b.strands(), off, reinterpret_cast<const int4 *>(ab.rows), ab.anchor_chain, ab.anchor_pred, coff,
                        reinterpret_cast<const int4 *>(ab.chains), (long long)U, cap,
                        ctg.n_contigs > 0 ? reinterpret_cast<const long long *>(ctg.offsets) : nullptr, (int)ctg.n_contigs};
    const long long want = (cap + kAlnWaves - 1) / kAlnWaves, most = (long long)(ix->num_cus > 0 ? ix->num_cus : 256) * 4;
    LAUNCH(align_kernel, dim3((unsigned)std::min(want, most)), dim3(kAlnWaves * kWave), 0, s, ix->dev, in, prm,
           static_cast<const int32_t *>(a.unit), reinterpret_cast<int4 *>(d_aln));
    if (d_totals)
        LAUNCH(align_totals_kernel, dim3(1), dim3(kScanBlock), 0, s, coff, (long long)U, cap, reinterpret_cast<const int4 *>(d_aln),
               reinterpret_cast<long long *>(d_totals));
    return GENIE_OK;
}

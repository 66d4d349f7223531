// sam_text.inc -- genie_sam_text: the SAM records of a mapped batch as bytes in device memory, with the NM, AS, MD, MC and MQ tags
// (included by kernels.hip behind windows.inc, inside namespace genie).  The definition is the header's; DESIGN.md section 28
// has the reasoning.
//
// A line is a read's record, or the unmapped line of a read without records; line l of read r is its (l - first(r))-th record,
// first(r) = min(so[r], R) + (reads before r without records).  One wave writes one line: sam_line walks the fields in their
// order with a cursor that is the same in every lane, the lanes over the bytes of a name, of SEQ and QUAL, over the digits of a
// number and over the ops of a CIGAR, 64 at a time.  With kWrite == false the same walk only adds the lengths up, and loads no
// read, no name and no reference base.
//   ST0 chain_check_kernel x 4, sam_cigar_check_kernel   the five offset arrays; the host reads the flag: the call's one
//                           synchronisation
//   ST1 sam_empty_kernel    one lane per read: 1 for a read without records
//   ST2 launch_compact      those marks scanned: the reads without records before every read
//   ST3 sam_table_kernel    one lane per read and per record: the (read, record or -1) of its line
//   ST4 sam_line_kernel<false>  one wave per line, grid-stride: its length
//   ST5 launch_compact      the lengths scanned into the line offsets
//   ST6 sam_finish_kernel   entries 0 .. n_lines of d_line_offsets, and the three totals
//   ST7 sam_line_kernel<true>   the same walk with the stores, every one of them below min(the line's end, cap_text)
// The text of an op is its length's digits and a letter; where it goes is a wave prefix sum over the ops' text lengths, chunk
// after chunk of 64 ops with the running position carried.  MD's count in front of an X or a D is the sum of the = lengths since
// the last X or D: the prefix sum of the = lengths less its value at the last X or D before, which is a prefix MAXIMUM because
// that sum never falls; the reference position of an op is a third prefix sum.  The carries between chunks are the count so
// far, the reference position and the text position.
namespace {

constexpr int kSamWaves = 4;                                  // waves per block
constexpr int kSamTagNM = GENIE_SAM_NM, kSamTagAS = GENIE_SAM_AS, kSamTagMD = GENIE_SAM_MD, kSamTagMC = GENIE_SAM_MC, kSamTagMQ = GENIE_SAM_MQ;
constexpr int kSamOpI = 1, kSamOpD = 2, kSamOpEq = 7, kSamOpX = 8;

struct SamInput {
    const uint8_t *bases;
    const long long *ro;                  // d_read_offsets
    const uint8_t *quals;                 // or null
    long long N;
    const long long *so;                  // d_sel_offsets
    const int4 *rec;                      // three to a record
    long long n_records;
    const int4 *sam;                      // or null: single-end mode
    const int4 *info;                     // two to a record
    const long long *co;                  // d_cigar_offsets
    const uint32_t *cigar;
    const uint8_t *names;
    const long long *no;
    const uint8_t *cnames;
    const long long *cno;
    const long long *ctg;                 // or null: one contig [0, n)
    int nctg;                             // names there are: max(n_contigs, 1)
    int tags, flags;
};

struct SamArea {
    int *flag;                            // ST0's verdict
    int32_t *empty;                       // per read: 1 without records
    long long *eoff;                      // N + 1: the reads without records before read r
    int2 *table;                          // per line: (read, record or -1)
    int32_t *len;                         // per line
    long long *loff;                      // N + n_records + 1
    uint8_t *scan_tmp;                    // launch_compact's
};

inline int64_t sam_layout(uint8_t *base, int64_t N, int64_t n_records, SamArea *a)
{
    const int64_t L = N + n_records;
    Carver c{base};
    c.take(a->flag, 8);
    c.take(a->empty, N * 4);
    c.take(a->eoff, (N + 1) * 8);
    c.take(a->table, L * 8);
    c.take(a->len, L * 4);
    c.take(a->loff, (L + 1) * 8);
    c.take(a->scan_tmp, compact_tmp_bytes(L));
    return c.at;
}

__device__ __forceinline__ long long sam_record_count(const SamInput &in) { return sel_clamp(in.so[in.N], 0, in.n_records); }

// the cigar offsets: R + 1 entries, R known on the device only
__global__ void __launch_bounds__(256) sam_cigar_check_kernel(SamInput in, long long n_ops, int *__restrict__ flag)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x, R = sam_record_count(in);
    if (j > R) return;
    const long long o = in.co[j];
    bool bad = o < 0 || o > n_ops || (j == 0 && o != 0);
    if (j < R) {
        const long long o2 = in.co[j + 1];
        bad = bad || o2 < o || o2 - o > 0x7fffffffll;
    }
    if (bad) atomicOr(flag, 1);
}

// the records [a, b) of read r
__device__ __forceinline__ void sam_range(const SamInput &in, long long R, long long r, long long *a, long long *b)
{
    *a = sel_clamp(in.so[r], 0, R);
    *b = sel_clamp(in.so[r + 1], *a, R);
}

__global__ void __launch_bounds__(256) sam_empty_kernel(SamInput in, int32_t *__restrict__ empty)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= in.N) return;
    long long a, b;
    sam_range(in, sam_record_count(in), r, &a, &b);
    empty[r] = b == a ? 1 : 0;
}

__global__ void __launch_bounds__(256) sam_table_kernel(SamInput in, const long long *__restrict__ eoff, int2 *__restrict__ table)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x, R = sam_record_count(in);
    if (i < in.N) {
        long long a, b;
        sam_range(in, R, i, &a, &b);
        if (b == a) table[a + eoff[i]] = make_int2((int)i, -1);
        return;
    }
    const long long j = i - in.N;
    if (j >= R) return;
    long long lo = 0, hi = in.N;                                     // the last r in [0, N) with so[r] <= j
    while (lo < hi - 1) {
        const long long mid = (lo + hi) >> 1;
        if (in.so[mid] <= j) lo = mid; else hi = mid;
    }
    table[j + eoff[lo]] = make_int2((int)lo, (int)j);
}

// ------------------------------------------------------------------ the pieces of a line
__device__ __forceinline__ int sam_digits32(uint32_t u)
{
    int n = 1;
    n += u >= 10u;
    n += u >= 100u;
    n += u >= 1000u;
    n += u >= 10000u;
    n += u >= 100000u;
    n += u >= 1000000u;
    n += u >= 10000000u;
    n += u >= 100000000u;
    n += u >= 1000000000u;
    return n;
}

__device__ __forceinline__ int sam_digits(unsigned long long u)
{
    if ((u >> 32) == 0) return sam_digits32((uint32_t)u);
    int n = 10;
    unsigned long long p = 10000000000ull;
    while (n < 20 && u >= p) {
        n++;
        p *= 10ull;
    }
    return n;
}

// A condition that is the same in every lane, told to the compiler: the branch on it is a scalar branch and saves no mask.
// The walk's many branches are all of this kind; taken as divergent, their saved masks alone overflow the scalar registers.
__device__ __forceinline__ bool sam_all(bool c) { return rfl(c ? 1 : 0) != 0; }

template <bool kWrite>
struct SamOut {
    uint8_t *text;
    long long lim;                        // min(the line's end, cap_text): no store at or past it
    int lane;
    __device__ __forceinline__ void put(long long p, int ch) const
    {
        if (kWrite && p < lim) text[p] = (uint8_t)ch;
    }
};

// one lane writes u, nd digits, at p: divisions by the constant ten only
template <bool kWrite>
__device__ __forceinline__ void sam_put_number32(const SamOut<kWrite> &o, long long p, uint32_t u, int nd)
{
    if (!kWrite) return;
    for (int k = nd - 1; k >= 0; k--) {
        o.put(p + k, '0' + (int)(u % 10u));
        u /= 10u;
    }
}

template <bool kWrite>
__device__ __forceinline__ void sam_put_number64(const SamOut<kWrite> &o, long long p, unsigned long long u, int nd)
{
    if (!kWrite) return;
    for (; nd > 0 && (u >> 32) != 0; nd--) {
        o.put(p + nd - 1, '0' + (int)(u % 10ull));
        u /= 10ull;
    }
    sam_put_number32(o, p, (uint32_t)u, nd);
}

// the wave writes v in decimal, a lane per character -> the position behind it
template <bool kWrite>
__device__ __forceinline__ long long sam_dec(const SamOut<kWrite> &o, long long pos, int v)
{
    const bool neg = v < 0;
    const uint32_t u = neg ? 0u - (uint32_t)v : (uint32_t)v;
    const int len = sam_digits32(u) + (neg ? 1 : 0);
    if (kWrite && o.lane < len) {
        uint32_t w = u;
        for (int k = len - 1 - o.lane; k > 0; k--) w /= 10u;         // this lane's digit is the last of w
        o.put(pos + o.lane, neg && o.lane == 0 ? '-' : '0' + (int)(w % 10u));
    }
    return pos + len;
}

template <bool kWrite>
__device__ __forceinline__ long long sam_char(const SamOut<kWrite> &o, long long pos, int ch)
{
    if (kWrite && o.lane == 0) o.put(pos, ch);
    return pos + 1;
}

// up to eight characters, the first in the low byte
template <bool kWrite>
__device__ __forceinline__ long long sam_chars(const SamOut<kWrite> &o, long long pos, unsigned long long packed, int n)
{
    if (kWrite && o.lane < n) o.put(pos + o.lane, (int)((packed >> (8 * o.lane)) & 0xffu));
    return pos + n;
}

#define SAM_C(c, k) ((unsigned long long)(unsigned char)(c) << (8 * (k)))
#define SAM_TAG(a, b, t) (SAM_C('\t', 0) | SAM_C(a, 1) | SAM_C(b, 2) | SAM_C(':', 3) | SAM_C(t, 4) | SAM_C(':', 5))

// the bytes [lo, hi) of a CSR of bytes
template <bool kWrite>
__device__ __forceinline__ long long sam_bytes(const SamOut<kWrite> &o, long long pos, const uint8_t *src, long long lo, long long hi)
{
    const long long n = hi > lo ? hi - lo : 0;
    if (kWrite)
        for (long long i = o.lane; i < n; i += kWave) o.put(pos + i, src[lo + i]);
    return pos + n;
}

template <bool kWrite>
__device__ __forceinline__ long long sam_contig_name(const SamOut<kWrite> &o, const SamInput &in, long long pos, int contig)
{
    const long long c = sel_clamp(contig, 0, in.nctg - 1);
    return sam_bytes(o, pos, in.cnames, in.cno[c], in.cno[c + 1]);
}

__device__ __forceinline__ int sam_op_letter(uint32_t code)
{
    if (code >= 8u) return code == 8u ? 'X' : '?';
    return (int)((0x3d5048534e44494dull >> (8 * code)) & 0xffu);     // MIDNSHP=
}

__device__ __forceinline__ int sam_base_letter(uint32_t code) { return code < 4u ? (int)((0x54474341u >> (8 * code)) & 0xffu) : 'N'; }

__device__ __forceinline__ unsigned long long sam_shfl64(unsigned long long v, int src)
{
    const unsigned int lo = (unsigned)__shfl((int)(unsigned)v, src, kWave);
    const unsigned int hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, kWave);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long sam_inclusive_max64(unsigned long long v, int lane)
{
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const unsigned int lo = (unsigned)__shfl_up((int)(unsigned)v, off, kWave);
        const unsigned int hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), off, kWave);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        if (lane >= off && w > v) v = w;
    }
    return v;
}

// the ops [lo, hi) as CIGAR text, `*` for none
template <bool kWrite>
__device__ __forceinline__ long long sam_cigar(const SamOut<kWrite> &o, const SamInput &in, long long pos, long long lo, long long hi)
{
    const int chunks = rfl((int)((hi - lo + kWave - 1) / kWave));        // at most 2^31 - 1 ops: the offsets were checked
    if (chunks <= 0) return sam_char(o, pos, '*');
    for (int ch = 0; ch < chunks; ch++) {
        const long long k = lo + (long long)ch * kWave + o.lane;
        const uint32_t op = k < hi ? in.cigar[k] : 0u;
        const int nd = sam_digits32(op >> 4);
        const unsigned long long mine = k < hi ? (unsigned long long)(nd + 1) : 0ull;
        if (kWrite) {
            const unsigned long long inc = wave_inclusive_scan64(mine, o.lane);
            if (k < hi) {
                const long long p = pos + (long long)(inc - mine);
                sam_put_number32(o, p, op >> 4, nd);
                o.put(p + nd, sam_op_letter(op & 15u));
            }
            pos += (long long)sam_shfl64(inc, kWave - 1);
        } else {
            pos += (long long)wave_sum64(mine);
        }
    }
    return pos;
}

// the packed reference and its length: all that the letters of MD need of the index
struct SamRef {
    const RefRec *ref;
    int n;
};

__device__ __forceinline__ int sam_ref_letter(const SamRef &ix, long long t)
{
    t = sel_clamp(t, 0, (long long)ix.n - 1);
    const uint64_t w = reinterpret_cast<const uint64_t *>(ix.ref)[(t >> 5) * 2];
    return sam_base_letter((uint32_t)(w >> (62 - 2 * (int)(t & 31))) & 3u);
}

// MD of the ops [lo, hi), the first of them at reference position t
template <bool kWrite>
__device__ __forceinline__ long long sam_md(const SamOut<kWrite> &o, const SamRef &ix, const SamInput &in, long long pos, long long lo,
                                            long long hi, long long t)
{
    unsigned long long count = 0;                                    // c so far
    const int chunks = rfl((int)((hi - lo + kWave - 1) / kWave));
    for (int ch = 0; ch < chunks; ch++) {
        const long long k = lo + (long long)ch * kWave + o.lane;
        const uint32_t op = k < hi ? in.cigar[k] : 0u;
        const uint32_t code = op & 15u, L = op >> 4;
        const bool is_x = code == kSamOpX && L > 0, is_d = code == kSamOpD, brk = is_x || is_d;
        const unsigned long long eq = code == kSamOpEq ? L : 0u;
        const unsigned long long E = wave_inclusive_scan64(eq, o.lane);
        // E at the last X or D before this op, plus one; 0 for none
        const unsigned long long mx = sam_inclusive_max64(brk ? E + 1 : 0ull, o.lane);
        unsigned long long before = sam_shfl64(mx, o.lane > 0 ? o.lane - 1 : 0);
        if (o.lane == 0) before = 0;
        const unsigned long long c = before ? E - eq - (before - 1) : count + E - eq;
        const int nd = sam_digits(c);
        const unsigned long long mine = is_x ? (unsigned long long)nd + 1 + 2ull * (L - 1) : (is_d ? (unsigned long long)nd + 1 + L : 0ull);
        const unsigned long long all_mx = sam_shfl64(mx, kWave - 1), all_E = sam_shfl64(E, kWave - 1);
        count = all_mx ? all_E - (all_mx - 1) : count + all_E;
        if (kWrite) {
            const unsigned long long span = (code == kSamOpEq || code == kSamOpX || code == kSamOpD) ? L : 0u;
            const unsigned long long T = wave_inclusive_scan64(span, o.lane), P = wave_inclusive_scan64(mine, o.lane);
            if (brk) {
                long long p = pos + (long long)(P - mine);
                const long long at = t + (long long)(T - span);
                sam_put_number64(o, p, c, nd);
                p += nd;
                if (is_d) {
                    o.put(p, '^');
                    for (uint32_t i = 0; i < L && p + 1 + i < o.lim; i++) o.put(p + 1 + i, sam_ref_letter(ix, at + i));
                } else {
                    o.put(p, sam_ref_letter(ix, at));
                    for (uint32_t i = 1; i < L && p + 2 * i - 1 < o.lim; i++) {
                        o.put(p + 2 * i - 1, '0');
                        o.put(p + 2 * i, sam_ref_letter(ix, at + i));
                    }
                }
            }
            t += (long long)sam_shfl64(T, kWave - 1);
            pos += (long long)sam_shfl64(P, kWave - 1);
        } else {
            pos += (long long)wave_sum64(mine);
        }
    }
    const int nd = sam_digits(count);
    if (o.lane == 0) sam_put_number64(o, pos, count, nd);
    return pos + nd;
}

// SEQ and QUAL of read r with the tabs in front of them: turned for strand 1
template <bool kWrite>
__device__ __forceinline__ long long sam_seq_qual(const SamOut<kWrite> &o, const SamInput &in, long long pos, long long r, bool turned)
{
    if (sam_all((in.flags & GENIE_SAM_NO_SEQ) != 0)) return sam_chars(o, pos, SAM_C('\t', 0) | SAM_C('*', 1) | SAM_C('\t', 2) | SAM_C('*', 3), 4);
    const long long b0 = in.ro[r], L = in.ro[r + 1] > b0 ? in.ro[r + 1] - b0 : 0;
    pos = sam_char(o, pos, '\t');
    if (kWrite)
        for (long long i = o.lane; i < L; i += kWave) {
            uint32_t code = in.bases[b0 + (turned ? L - 1 - i : i)];
            if (turned && code < 4u) code = 3u - code;
            o.put(pos + i, sam_base_letter(code));
        }
    pos = sam_char(o, pos + L, '\t');
    if (sam_all(in.quals == nullptr)) return sam_char(o, pos, '*');
    if (kWrite)
        for (long long i = o.lane; i < L; i += kWave) o.put(pos + i, in.quals[b0 + (turned ? L - 1 - i : i)]);
    return pos + L;
}

// the last record of read r whose flag has neither 0x100 nor 0x800, or -1: the same in every lane
__device__ __forceinline__ long long sam_chosen(const SamInput &in, long long R, long long r, int lane)
{
    long long a, b;
    sam_range(in, R, r, &a, &b);
    const int chunks = rfl((int)((b - a + kWave - 1) / kWave));
    for (int ch = 0; ch < chunks; ch++) {
        const long long top = b - (long long)ch * kWave, k = top - 1 - lane;
        const unsigned long long hit = __ballot(k >= a && (in.sam[k].x & 0x900) == 0);
        if (hit) return top - 1 - (__ffsll((long long)hit) - 1);
    }
    return -1;
}

// What a line says of its record j of read r, or with j < 0 of the read without records: the columns that the text and the BAM
// record (bam_records.inc) share, derived in this one place
struct SamFields {
    long long mate;                       // the mate's chosen record, or -1
    int flag, mapq, contig, rpos, tlen, strand;
};

__device__ __forceinline__ SamFields sam_fields(const SamInput &in, long long R, long long r, long long j, int lane)
{
    const bool paired = sam_all(in.sam != nullptr), mapped = sam_all(j >= 0);
    long long mate = -1;
    int flag, mapq = 0, contig = 0, rpos = 0, tlen = 0, strand = 0;
    if (mapped) {
        const int4 r0 = in.rec[3 * j], r1 = in.rec[3 * j + 1];
        strand = r0.w != 0 ? 1 : 0;
        contig = r1.x;
        rpos = r1.y;
        if (paired) {
            const int4 f = in.sam[j];
            flag = f.x;
            mapq = f.y;
            mate = f.z >= 0 && f.z < R ? f.z : -1;
            tlen = f.w;
        } else {
            flag = (strand ? 0x10 : 0) | (r0.z == 1 ? 0x800 : 0) | (r0.z == 2 ? 0x100 : 0);
            mapq = in.rec[3 * j + 2].w;
        }
    } else if (paired) {
        flag = 0x1 | 0x4 | ((r & 1) ? 0x80 : 0x40);
        mate = sam_chosen(in, R, r ^ 1, lane);
        if (sam_all(mate < 0)) {
            flag |= 0x8;
        } else {
            if (in.rec[3 * mate].w != 0) flag |= 0x20;
            const int4 m1 = in.rec[3 * mate + 1];
            contig = m1.x;
            rpos = m1.y;
        }
    } else {
        flag = 0x4;
    }
    return SamFields{mate, flag, mapq, contig, rpos, tlen, strand};
}

// The line of read r: its record j, or with j < 0 its unmapped line.  -> the position behind its line end
template <bool kWrite>
__device__ __forceinline__ long long sam_line(const SamRef &ix, const SamInput &in, long long R, long long r, long long j,
                                              const SamOut<kWrite> &o, long long pos)
{
    const bool paired = sam_all(in.sam != nullptr), mapped = sam_all(j >= 0);
    const int tags = rfl(in.tags);
    const SamFields f = sam_fields(in, R, r, j, o.lane);
    const long long mate = f.mate;
    const int flag = f.flag, mapq = f.mapq, contig = f.contig, rpos = f.rpos, tlen = f.tlen, strand = f.strand;
    const bool mated = sam_all(mate >= 0), placed = mapped || mated;                        // RNAME and POS are some record's
    pos = sam_bytes(o, pos, in.names, in.no[r], in.no[r + 1]);
    pos = sam_char(o, pos, '\t');
    pos = sam_dec(o, pos, flag);
    pos = sam_char(o, pos, '\t');
    pos = placed ? sam_contig_name(o, in, pos, contig) : sam_char(o, pos, '*');
    pos = sam_char(o, pos, '\t');
    pos = sam_dec(o, pos, rpos);
    pos = sam_char(o, pos, '\t');
    pos = sam_dec(o, pos, mapq);
    pos = sam_char(o, pos, '\t');
    const long long c_lo = mapped ? in.co[j] : 0, c_hi = mapped ? in.co[j + 1] : 0;
    pos = sam_cigar(o, in, pos, c_lo, c_hi);
    pos = sam_char(o, pos, '\t');
    int pnext = 0;
    if (!mapped) {
        pos = sam_char(o, pos, mated ? '=' : '*');
        pnext = rpos;
    } else if (mated) {
        const int4 m1 = in.rec[3 * mate + 1];
        pos = sam_all(m1.x == contig) ? sam_char(o, pos, '=') : sam_contig_name(o, in, pos, m1.x);
        pnext = m1.y;
    } else {
        pos = sam_char(o, pos, '*');
    }
    pos = sam_char(o, pos, '\t');
    pos = sam_dec(o, pos, pnext);
    pos = sam_char(o, pos, '\t');
    pos = sam_dec(o, pos, tlen);
    pos = sam_seq_qual(o, in, pos, r, mapped && strand != 0);
    if (mapped) {
        if (tags & kSamTagNM) {
            pos = sam_chars(o, pos, SAM_TAG('N', 'M', 'i'), 6);
            pos = sam_dec(o, pos, in.info[2 * j].w);
        }
        if (tags & kSamTagAS) {
            pos = sam_chars(o, pos, SAM_TAG('A', 'S', 'i'), 6);
            pos = sam_dec(o, pos, in.rec[3 * j + 2].y);
        }
        if ((tags & kSamTagMD) && sam_all(c_hi > c_lo)) {
            long long start = 0;
            if (sam_all(in.ctg != nullptr)) {
                const long long c = sel_clamp(contig, 0, (long long)in.nctg - 1);
                start = sel_clamp(in.ctg[c], 0, ix.n);
            }
            pos = sam_chars(o, pos, SAM_TAG('M', 'D', 'Z'), 6);
            pos = sam_md(o, ix, in, pos, c_lo, c_hi, start + (long long)rpos - 1);
        }
    }
    if (paired && mated) {
        const long long m_lo = in.co[mate], m_hi = in.co[mate + 1];
        if ((tags & kSamTagMC) && sam_all(m_hi > m_lo)) {
            pos = sam_chars(o, pos, SAM_TAG('M', 'C', 'Z'), 6);
            pos = sam_cigar(o, in, pos, m_lo, m_hi);
        }
        if (tags & kSamTagMQ) {
            pos = sam_chars(o, pos, SAM_TAG('M', 'Q', 'i'), 6);
            pos = sam_dec(o, pos, in.sam[mate].y);
        }
    }
    return sam_char(o, pos, '\n');
}

#undef SAM_TAG
#undef SAM_C

// One wave per line, grid-stride.  kWrite: the bytes of [loff[l], loff[l + 1]) below cap_text; else len[l], and 0 for the
// places of the table past the last line.  The arguments are some fifty scalar registers, all of them live across the whole
// walk, and the walk's own wave-wide values and saved masks come on top: held in scalar registers they do not fit.  So the
// block stages them in LDS and every use reads them from there into a vector register, of which there are plenty.
struct SamJob {
    SamRef ref;
    SamInput in;
    const long long *eoff;
    const int2 *table;
    long long bound;
    int32_t *len;
    const long long *loff;
    uint8_t *text;
    long long cap_text;
};

template <bool kWrite>
__global__ void __launch_bounds__(kSamWaves *kWave) sam_line_kernel(SamJob job)
{
    __shared__ SamJob staged;
    if (threadIdx.x == 0) staged = job;
    __syncthreads();
    const SamJob &g = staged;
    const SamInput &in = g.in;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long long R = sam_record_count(in), n_lines = R + sel_clamp(g.eoff[in.N], 0, in.N);
    const long long end = kWrite ? n_lines : g.bound;
    for (long long l = (long long)blockIdx.x * kSamWaves + wave; sam_all(l < end); l += (long long)gridDim.x * kSamWaves) {
        // the staged arguments are read again for every line: what is derived from them is then derived where it is used, not
        // once in front of the loop and held in scalar registers through all of it
        asm volatile("" ::: "memory");
        if (!kWrite && sam_all(l >= n_lines)) {
            if (lane == 0) g.len[l] = 0;
            continue;
        }
        const int2 e = g.table[l];
        const long long r = sel_clamp(e.x, 0, in.N - 1), j = e.y >= 0 && e.y < R ? e.y : -1;
        if (kWrite) {
            const long long first = g.loff[l], last = g.loff[l + 1], cap = g.cap_text;
            if (sam_all(first >= cap)) continue;
            const SamOut<true> o{g.text, last < cap ? last : cap, lane};
            sam_line<true>(g.ref, in, R, r, j, o, first);
        } else {
            const SamOut<false> o{nullptr, 0, lane};
            const long long n = sam_line<false>(g.ref, in, R, r, j, o, 0);
            if (lane == 0) g.len[l] = (int32_t)sel_clamp(n, 0, 0x7fffffffll);
        }
    }
}

__global__ void __launch_bounds__(256) sam_finish_kernel(SamInput in, const long long *__restrict__ eoff, const long long *__restrict__ loff,
                                                         long long bound, long long *__restrict__ line_offsets,
                                                         long long *__restrict__ totals)
{
    const long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long unmapped = sel_clamp(eoff[in.N], 0, in.N), n_lines = sam_record_count(in) + unmapped;
    if (l <= n_lines) line_offsets[l] = loff[l];
    if (l == 0 && totals) {
        totals[0] = n_lines;
        totals[1] = loff[bound];
        totals[2] = unmapped;
    }
}

// the batch as the kernels take it
inline SamInput sam_input(const ContigTable &ctg, const SamBatch &b)
{
    const long long nc = ctg.n_contigs > 0 ? ctg.n_contigs : 1;
    return SamInput{b.bases, reinterpret_cast<const long long *>(b.read_offsets), b.quals, (long long)b.N,
                    reinterpret_cast<const long long *>(b.sel_offsets), reinterpret_cast<const int4 *>(b.records), (long long)b.n_records,
                    reinterpret_cast<const int4 *>(b.sam), reinterpret_cast<const int4 *>(b.info),
                    reinterpret_cast<const long long *>(b.cigar_offsets), b.cigar, b.names,
                    reinterpret_cast<const long long *>(b.name_offsets), b.contig_names,
                    reinterpret_cast<const long long *>(b.contig_name_offsets),
                    ctg.n_contigs > 0 ? reinterpret_cast<const long long *>(ctg.offsets) : nullptr, (int)nc, b.tags, b.flags};
}

// ST0 .. ST3 for N > 0: the offset checks with the call's one synchronisation, then a.eoff and a.table
inline int sam_tables(const SamInput &in, const SamBatch &b, const SamArea &a, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = b.N, n_rec = b.n_records, bound = N + n_rec;
    const long long nc = in.nctg;
    HIP_TRY(hipMemsetAsync(a.flag, 0, 8, s));
    LAUNCH_BLOCKS(chain_check_kernel, (N + 1 + 255) / 256, 256, 0, s, in.ro, (long long)N, (long long)b.total_bases, a.flag);
    LAUNCH_BLOCKS(chain_check_kernel, (N + 1 + 255) / 256, 256, 0, s, in.so, (long long)N, 0x7fffffffffffffffll, a.flag);
    LAUNCH_BLOCKS(chain_check_kernel, (N + 1 + 255) / 256, 256, 0, s, in.no, (long long)N, (long long)b.name_bytes, a.flag);
    LAUNCH_BLOCKS(chain_check_kernel, (nc + 1 + 255) / 256, 256, 0, s, in.cno, nc, (long long)b.contig_name_bytes, a.flag);
    if (n_rec > 0) LAUNCH_BLOCKS(sam_cigar_check_kernel, (n_rec + 1 + 255) / 256, 256, 0, s, in, (long long)b.n_ops, a.flag);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, a.flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return GENIE_E_INVALID;
    LAUNCH_BLOCKS(sam_empty_kernel, (N + 255) / 256, 256, 0, s, in, a.empty);
    if (int rc = launch_compact(a.empty, nullptr, N, 1, reinterpret_cast<int64_t *>(a.eoff), nullptr, 0, a.scan_tmp, stream)) return rc;
    const long long *eoff = a.eoff;
    LAUNCH_BLOCKS(sam_table_kernel, (bound + 255) / 256, 256, 0, s, in, eoff, a.table);
    return GENIE_OK;
}

}  // namespace

int64_t sam_text_workspace_bytes(int64_t N, int64_t n_records)
{
    SamArea a;
    return sam_layout(nullptr, N, n_records, &a);
}

int launch_sam_text(const genie_index *ix, const ContigTable &ctg, const SamBatch &b, const SamTextOut &out, void *ws, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = b.N, n_rec = b.n_records, bound = N + n_rec;
    if (N == 0) {
        HIP_TRY(hipMemsetAsync(out.line_offsets, 0, 8, s));
        if (out.totals) HIP_TRY(hipMemsetAsync(out.totals, 0, 24, s));
        return GENIE_OK;
    }
    SamArea a;
    sam_layout(static_cast<uint8_t *>(ws), N, n_rec, &a);
    const SamInput in = sam_input(ctg, b);
    if (int rc = sam_tables(in, b, a, stream)) return rc;
    const long long *eoff = a.eoff;
    const int2 *table = a.table;
    const long long want = (bound + kSamWaves - 1) / kSamWaves, most = (long long)(ix->num_cus > 0 ? ix->num_cus : 256) * 8;
    const dim3 grid((unsigned)std::min(want, most)), block(kSamWaves * kWave);
    const SamRef ref{ix->dev.ref, ix->dev.n};
    const SamJob job{ref, in, eoff, table, (long long)bound, a.len, a.loff, out.text, (long long)out.cap_text};
    LAUNCH(sam_line_kernel<false>, grid, block, 0, s, job);
    if (int rc = launch_compact(a.len, nullptr, bound, 0x7FFFFFFF, reinterpret_cast<int64_t *>(a.loff), nullptr, 0, a.scan_tmp, stream))
        return rc;
    const long long *loff = a.loff;
    LAUNCH_BLOCKS(sam_finish_kernel, (bound + 1 + 255) / 256, 256, 0, s, in, eoff, loff, (long long)bound,
                  reinterpret_cast<long long *>(out.line_offsets), reinterpret_cast<long long *>(out.totals));
    if (out.text && out.cap_text > 0)
        LAUNCH(sam_line_kernel<true>, grid, block, 0, s, job);
    return GENIE_OK;
}

// bam_records.inc -- genie_bam_records: the uncompressed BAM alignment records of a mapped batch as bytes in device memory
// (included by kernels.hip behind sam_text.inc, inside namespace genie).  The definition is the header's; DESIGN.md section 31
// has the reasoning.
//
// One record per line of genie_sam_text, in its order, from the same inputs: the table of lines (ST0 .. ST3), the columns of a
// line (sam_fields), the texts of MD and MC (sam_md, sam_cigar), the bounded store (SamOut) and the staged arguments (SamJob)
// are sam_text.inc's.  One wave writes one record.  Where every field lies is known before a byte is written: the head has 36
// bytes, the name, the ops, SEQ and QUAL have lengths that are sums of the inputs' own, and only the Z tags MD and MC must be
// walked.  So the sizing pass loads no op unless one of those two is asked for.
//   ST0 .. ST3                as sam_text.inc
//   BT4 bam_record_kernel<false>  one wave per record, grid-stride: its length
//   BT5 launch_compact        the lengths scanned into the record offsets
//   BT6 sam_finish_kernel     entries 0 .. n of d_record_offsets, and the three totals
//   BT7 bam_record_kernel<true>   the stores, every one of them below min(the record's end, cap_data)
// A record starts at any byte, so nothing is stored wider than a byte: a lane stores one byte, the lanes of a step consecutive
// ones.  The ops go out four steps to a chunk of 64, lane i of step q writing byte 64 q + i of the chunk's 256, its op fetched
// from lane (64 q + i) / 4; the same loop sums the reference span that `bin` needs, so the head is written last.  SEQ is one
// byte, two bases, per lane; on the reverse strand the bases L - 1 - 2 i and L - 2 - 2 i, complemented.
namespace {

constexpr int kBamHead = 36;                                  // block_size .. tlen
constexpr long long kBamMaxOps = 65535;                       // more go into the CG tag

// a tag of type i: two letters, `i`, an int32
template <bool kWrite>
__device__ __forceinline__ long long bam_tag_i(const SamOut<kWrite> &o, long long pos, int a, int b, int v)
{
    return sam_chars(o, pos, (unsigned long long)a | ((unsigned long long)b << 8) | ((unsigned long long)'i' << 16) |
                              ((unsigned long long)(uint32_t)v << 24), 7);
}

__device__ __forceinline__ uint32_t bam_nibble(uint32_t code, bool turned)
{
    if (code >= 4u) return 15u;
    return 1u << (turned ? 3u - code : code);
}

// SAMv1's reg2bin on int64 with arithmetic shifts, cut to 16 bits
__device__ __forceinline__ uint32_t bam_bin(long long beg, long long end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14)) & 0xffffu;
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17)) & 0xffffu;
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20)) & 0xffffu;
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23)) & 0xffffu;
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26)) & 0xffffu;
    return 0u;
}

// The record of read r: its record j, or with j < 0 its unmapped record.  -> the position behind it.  `last` is the record's end
// as the sizing pass found it (kWrite only): block_size comes from it, so a record that was cut says the length it has.
template <bool kWrite>
__device__ __forceinline__ long long bam_record(const SamRef &ix, const SamInput &in, long long R, long long r, long long j,
                                                const SamOut<kWrite> &o, long long pos, long long last)
{
    const bool paired = sam_all(in.sam != nullptr), mapped = sam_all(j >= 0);
    const int tags = rfl(in.tags);
    const SamFields f = sam_fields(in, R, r, j, o.lane);
    const long long mate = f.mate;
    const bool mated = sam_all(mate >= 0), placed = mapped || mated, turned = mapped && f.strand != 0;
    const long long first = pos;
    // where the fields lie
    const long long n_lo = in.no[r], n_len = in.no[r + 1] > n_lo ? in.no[r + 1] - n_lo : 0;
    const int name = n_len > 254 ? 254 : (int)n_len, l_name = (name > 0 ? name : 1) + 1;
    const long long c_lo = mapped ? in.co[j] : 0, c_hi = mapped ? in.co[j + 1] : 0, n_ops = c_hi > c_lo ? c_hi - c_lo : 0;
    const bool big = sam_all(n_ops > kBamMaxOps);
    long long L = 0;
    const long long b0 = in.ro[r];
    if (sam_all((in.flags & GENIE_SAM_NO_SEQ) == 0)) L = in.ro[r + 1] > b0 ? in.ro[r + 1] - b0 : 0;
    const long long n_seq = (L + 1) >> 1;
    const long long p_name = first + kBamHead, p_cigar = p_name + l_name, p_seq = p_cigar + 4 * (big ? 2 : n_ops);
    const long long p_qual = p_seq + n_seq;
    pos = p_qual + L;
    if (kWrite) {
        if (sam_all(name > 0)) {
            for (int i = o.lane; i < name; i += kWave) o.put(p_name + i, in.names[n_lo + i]);
        } else {
            sam_char(o, p_name, '*');
        }
        sam_char(o, p_name + l_name - 1, 0);
        for (long long i = o.lane; i < n_seq; i += kWave) {
            const long long a = 2 * i;
            const uint32_t hi = bam_nibble(in.bases[b0 + (turned ? L - 1 - a : a)], turned);
            const uint32_t lo = a + 1 < L ? bam_nibble(in.bases[b0 + (turned ? L - 2 - a : a + 1)], turned) : 0u;
            o.put(p_seq + i, (int)(hi << 4 | lo));
        }
        if (sam_all(in.quals == nullptr)) {
            for (long long i = o.lane; i < L; i += kWave) o.put(p_qual + i, 0xff);
        } else {
            for (long long i = o.lane; i < L; i += kWave) {
                const int q = (int)in.quals[b0 + (turned ? L - 1 - i : i)] - 33;
                o.put(p_qual + i, q > 0 ? q : 0);
            }
        }
    }
    // the tags: NM, AS, MD, MC, MQ under the text's conditions
    if (mapped) {
        if (tags & kSamTagNM) pos = bam_tag_i(o, pos, 'N', 'M', in.info[2 * j].w);
        if (tags & kSamTagAS) pos = bam_tag_i(o, pos, 'A', 'S', in.rec[3 * j + 2].y);
        if ((tags & kSamTagMD) && sam_all(c_hi > c_lo)) {
            long long start = 0;
            if (sam_all(in.ctg != nullptr)) {
                const long long c = sel_clamp(f.contig, 0, (long long)in.nctg - 1);
                start = sel_clamp(in.ctg[c], 0, ix.n);
            }
            pos = sam_chars(o, pos, (unsigned long long)'M' | ((unsigned long long)'D' << 8) | ((unsigned long long)'Z' << 16), 3);
            pos = sam_md(o, ix, in, pos, c_lo, c_hi, start + (long long)f.rpos - 1);
            pos = sam_char(o, pos, 0);
        }
    }
    if (paired && mated) {
        const long long m_lo = in.co[mate], m_hi = in.co[mate + 1];
        if ((tags & kSamTagMC) && sam_all(m_hi > m_lo)) {
            pos = sam_chars(o, pos, (unsigned long long)'M' | ((unsigned long long)'C' << 8) | ((unsigned long long)'Z' << 16), 3);
            pos = sam_cigar(o, in, pos, m_lo, m_hi);
            pos = sam_char(o, pos, 0);
        }
        if (tags & kSamTagMQ) pos = bam_tag_i(o, pos, 'M', 'Q', in.sam[mate].y);
    }
    // the ops: into the cigar field, or behind CG B I and their count
    const long long p_ops = big ? pos + 8 : p_cigar;
    if (big) pos += 8 + 4 * n_ops;
    if (!kWrite) return pos;
    unsigned long long span = 0;                                     // of the reference: the ops with the codes 0, 2, 3, 7, 8
    const int chunks = rfl((int)((n_ops + kWave - 1) / kWave));      // at most 2^31 - 1 ops: the offsets were checked
    for (int ch = 0; ch < chunks; ch++) {
        const long long k0 = c_lo + (long long)ch * kWave, k = k0 + o.lane;
        const uint32_t op = k < c_hi ? in.cigar[k] : 0u;
        const uint32_t code = op & 15u;
        span += wave_sum64((code == 0u || code == 2u || code == 3u || code == 7u || code == 8u) ? (unsigned long long)(op >> 4) : 0ull);
        const long long at = p_ops + 4 * (long long)ch * kWave;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int idx = q * kWave + o.lane, src = idx >> 2;
            const uint32_t v = (uint32_t)__shfl((int)op, src, kWave);
            if (k0 + src < c_hi) o.put(at + idx, (int)((v >> (8 * (idx & 3))) & 0xffu));
        }
    }
    // the head
    const int nc = rfl(in.nctg);
    const int ref_id = placed ? (int)sel_clamp(f.contig, 0, nc - 1) : -1;
    int next_id = -1, pnext = 0;
    if (!mapped) {
        if (mated) next_id = ref_id;
        pnext = f.rpos;
    } else if (mated) {
        const int4 m1 = in.rec[3 * mate + 1];
        next_id = (int)sel_clamp(m1.x, 0, nc - 1);
        pnext = m1.y;
    }
    const int bpos = (int)((uint32_t)f.rpos - 1u), l_seq = (int)sel_clamp(L, 0, 0x7fffffffll);
    const long long beg = bpos, end = beg + (span ? (long long)span : 1ll);
    const uint32_t mapq = (uint32_t)sel_clamp(f.mapq, 0, 255), n_cigar = big ? 2u : (uint32_t)n_ops;
    if (big) {
        const unsigned long long cut = span < 0xfffffffull ? span : 0xfffffffull;
        sam_chars(o, p_cigar, (unsigned long long)((uint32_t)l_seq << 4 | 4u) | ((unsigned long long)((uint32_t)cut << 4 | 3u) << 32), 8);
        sam_chars(o, p_ops - 8, (unsigned long long)'C' | ((unsigned long long)'G' << 8) | ((unsigned long long)'B' << 16) |
                                 ((unsigned long long)'I' << 24) | ((unsigned long long)(uint32_t)n_ops << 32), 8);
    }
    const int w = o.lane >> 2;                                       // the head's word of this lane
    uint32_t word = (uint32_t)(last - first - 4);
    word = w == 1 ? (uint32_t)ref_id : word;
    word = w == 2 ? (uint32_t)bpos : word;
    word = w == 3 ? ((uint32_t)l_name | mapq << 8 | bam_bin(beg, end) << 16) : word;
    word = w == 4 ? (n_cigar | ((uint32_t)f.flag & 0xffffu) << 16) : word;
    word = w == 5 ? (uint32_t)l_seq : word;
    word = w == 6 ? (uint32_t)next_id : word;
    word = w == 7 ? (uint32_t)pnext - 1u : word;
    word = w == 8 ? (uint32_t)f.tlen : word;
    if (o.lane < kBamHead) o.put(first + o.lane, (int)((word >> (8 * (o.lane & 3))) & 0xffu));
    return pos;
}

// One wave per record, grid-stride: sam_line_kernel with the other walk.  job.text is d_data, job.cap_text cap_data.
template <bool kWrite>
__global__ void __launch_bounds__(kSamWaves *kWave) bam_record_kernel(SamJob job)
{
    __shared__ SamJob staged;
    if (threadIdx.x == 0) staged = job;
    __syncthreads();
    const SamJob &g = staged;
    const SamInput &in = g.in;
    const int wave = threadIdx.x / kWave;
    int lane = threadIdx.x & (kWave - 1);
    const long long R = sam_record_count(in), n_lines = R + sel_clamp(g.eoff[in.N], 0, in.N);
    const long long end = kWrite ? n_lines : g.bound;
    for (long long l = (long long)blockIdx.x * kSamWaves + wave; sam_all(l < end); l += (long long)gridDim.x * kSamWaves) {
        // as in sam_line_kernel: the staged arguments are read again for every record.  The lane passes through the barrier
        // too: the walk compares it with some twenty constants, and those masks, computed once in front of the loop and held
        // through all of it, are more scalar registers than there are
        asm volatile("" : "+v"(lane) : : "memory");
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
            bam_record<true>(g.ref, in, R, r, j, o, first, last);
        } else {
            const SamOut<false> o{nullptr, 0, lane};
            const long long n = bam_record<false>(g.ref, in, R, r, j, o, 0, 0);
            if (lane == 0) g.len[l] = (int32_t)sel_clamp(n, 0, 0x7fffffffll);
        }
    }
}

}  // namespace

int64_t bam_records_workspace_bytes(int64_t N, int64_t n_records)
{
    SamArea a;
    return sam_layout(nullptr, N, n_records, &a);
}

int launch_bam_records(const genie_index *ix, const ContigTable &ctg, const SamBatch &b, const SamTextOut &out, void *ws, void *stream)
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
    LAUNCH(bam_record_kernel<false>, grid, block, 0, s, job);
    if (int rc = launch_compact(a.len, nullptr, bound, 0x7FFFFFFF, reinterpret_cast<int64_t *>(a.loff), nullptr, 0, a.scan_tmp, stream))
        return rc;
    const long long *loff = a.loff;
    LAUNCH_BLOCKS(sam_finish_kernel, (bound + 1 + 255) / 256, 256, 0, s, in, eoff, loff, (long long)bound,
                  reinterpret_cast<long long *>(out.line_offsets), reinterpret_cast<long long *>(out.totals));
    if (out.text && out.cap_text > 0)
        LAUNCH(bam_record_kernel<true>, grid, block, 0, s, job);
    return GENIE_OK;
}

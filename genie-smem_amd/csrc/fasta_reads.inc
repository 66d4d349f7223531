// fasta_reads.inc -- genie_reads_from_fasta: FASTA text ('>' header lines, sequences wrapped over any number of lines) ->
// base codes back to back, int64 offsets and the text positions of the records (included by kernels.hip behind
// text_reads.inc, inside namespace genie; uses its tiles and its newline scan).  From ingest_tiles.inc: tile_count and
// tile_compact behind the classifier, tile_scan64 for fa_scan_kernel's three scans, the launch's tail.  Its own:
// fa_classify, what fa_scan_kernel makes of the scanned values, and the writer of a header's offset and record start.
//
// A read is the concatenation of many lines, so it is no slice of the text -- but reads lie back to back in d_bases, so
// d_bases is the STREAM COMPACTION of the text's kept bytes, and d_read_offsets[r] is the number of kept bytes in front of
// header r.  A byte is a CANDIDATE when it is no '\n', no '\r' in front of a '\n', its line does not start with '>' and, with
// GENIE_TEXT_PARTIAL, it lies in front of the last '\n' (the tail is no line).  A HEADER is a '>' at the start of a line (with
// GENIE_TEXT_PARTIAL: of a line that ends in this chunk).  A well-formed text has no candidate in front of its first
// header, so its kept bytes are its candidates (with GENIE_TEXT_PARTIAL: those in front of the last header).
// Three reads of the text, in tiles of kTrTile bytes, one block per tile, nothing per record and nothing per line:
//   FA1 tr_count_kernel, tr_scan_kernel (text_reads.inc)  the last newline before every tile, and of the text: where the
//                          line that crosses into a tile starts, hence whether it is a header line.
//   FA2 fa_count_kernel    per tile: candidates and headers; the tile position of its first and of its last header and the
//                          candidates in front of each; the largest number of candidates between two of its headers.
//       fa_scan_kernel     one block: exclusive sums of both counts over the tiles; an exclusive maximum scan of "candidates
//                          in front of the last header so far" (it never decreases) closes the reads that cross tiles, so
//                          the longest read needs no pass over the offsets and the sizing call knows it too.  Then the
//                          call's state: N, total_bases, longest read, consumed bytes, malformed or not.
//   FA3 fa_compact_kernel  tile_compact: a block scan of the lanes' (kept, header) counts places every code in an LDS image
//                          of the tile's run of d_bases and stores it as tr_translate_kernel does; the lane that holds a
//                          header's '>' writes d_read_offsets[r] and d_record_starts[r].
// No atomic anywhere: every output is a function of the text alone.  All positions are 64-bit.
namespace {

enum { kFaHeaders = kTrLines };                  // the state word tr_scan_kernel filled with the lines: here the headers

// Which of this lane's 16 bytes are candidates in front of `cut` (keep) and which are a header's '>' (mark).  c, prev0: the
// tile's newlines and the last newline before the tile.  Without GENIE_TEXT_PARTIAL cut = T; with it cut <= last_nl.
__device__ __forceinline__ TileLane fa_classify(const uint8_t *__restrict__ text, long long T, long long tile0, int c, long long prev0,
                                                int partial, long long last_nl, long long cut, const TrTile &s)
{
    const int t = threadIdx.x;
    TileLane out = {0u, 0u};
    const long long i0 = tile0 + 16 * t;
    if (i0 >= T) return out;
    int m = 0, hi = c;                                              // m = newlines of the tile before the lane's first byte
    while (m < hi) {
        const int mid = (m + hi) >> 1;
        if (s.nl[mid] < 16 * t) m = mid + 1; else hi = mid;
    }
    long long start = (m > 0 ? tile0 + s.nl[m - 1] : prev0) + 1;    // of the line the next byte belongs to
    bool header_line = false;
    if (start < i0)                                                 // the lane begins inside a line (start < i0 < T)
        header_line = (start >= tile0 ? tr_tile_byte(s, (int)(start - tile0)) : text[start]) == '>';
    const uint4 w = s.text[t];
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const long long i = i0 + k;
        if (i < 0 || i >= T) continue;
        const uint32_t b = (ws[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        if (b == '\n') {
            start = i + 1;
            continue;
        }
        if (i == start) {
            header_line = b == '>';
            if (header_line && (!partial || i < last_nl)) out.mark |= 1u << k;
        }
        if (header_line || i >= cut) continue;
        if (b == '\r') {                                            // dropped when a '\n' follows: one byte of look-ahead
            uint32_t next;
            if (k < 15) next = (ws[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xFFu;
            else if (t < kTrBlock - 1) next = tr_tile_byte(s, 16 * t + 16);
            else next = i + 1 < T ? text[i + 1] : 0u;               // across the tile's edge (tile bytes outside the text are 0)
            if (next == '\n') continue;
        }
        out.keep |= 1u << k;
    }
    return out;
}

__global__ void __launch_bounds__(kTrBlock) fa_count_kernel(const uint8_t *__restrict__ text, long long T, int lead, int partial,
                                                            const long long *__restrict__ last, const long long *__restrict__ state,
                                                            unsigned long long *__restrict__ cand, unsigned long long *__restrict__ hdrs,
                                                            TileInfo *__restrict__ info)
{
    __shared__ TrTile s;
    __shared__ TileMarks m;
    const long long tile = blockIdx.x;
    const int c = tr_load_tile(text, T, lead, tile, s);
    const long long last_nl = state[kTrLastNewline];
    const TileLane L = fa_classify(text, T, tile * kTrTile - lead, c, last[tile], partial, last_nl, partial ? last_nl : T, s);
    tile_count(L, s.wave_total, m, tile, cand, hdrs, info);
}

// single block: cand[], hdrs[] -> candidates / headers before each tile; then the call's state
__global__ void __launch_bounds__(kScanBlock) fa_scan_kernel(unsigned long long *__restrict__ cand, unsigned long long *__restrict__ hdrs,
                                                             const TileInfo *__restrict__ info, long long ntiles, long long T, int lead,
                                                             int partial, long long *__restrict__ state)
{
    constexpr int kWaves = kScanBlock / kWave;
    __shared__ long long wc[kWaves], wh[kWaves], wg[kWaves], wlen[kWaves], wpos[kWaves];
    __shared__ long long first_e;                                   // candidates in front of the first header
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) first_e = 0;
    // the carries, of the tiles so far: candidates, headers, candidates in front of the last header (-1: no header)
    long long carry_c = 0, carry_h = 0, carry_g = -1;
    long long longest = 0, last_header = -1;                        // this thread's share
    for (long long base = 0; base < ntiles; base += kScanBlock) {
        const long long i = base + threadIdx.x;
        const bool mine = i < ntiles;
        const long long c = mine ? (long long)cand[i] : 0ll, h = mine ? (long long)hdrs[i] : 0ll;
        TileInfo f = {0u, 0u, 0u, 0u};
        if (mine && h) f = info[i];
        const long long ex_c = tile_scan64<false>(c, carry_c, wc), ex_h = tile_scan64<false>(h, carry_h, wh);
        // candidates in front of the last header before this tile: an exclusive maximum scan, the value never decreases
        const long long g = tile_scan64<true>(h ? ex_c + f.before_last : -1ll, carry_g, wg);
        if (mine) {
            cand[i] = (unsigned long long)ex_c;
            hdrs[i] = (unsigned long long)ex_h;
            if (h) {
                const long long upto = ex_c + f.before_first;                // candidates in front of the tile's first header
                long long len = f.longest;
                if (g >= 0) len = upto - g > len ? upto - g : len;           // the read that the first header closes
                else first_e = upto;                                         // the text's first header: one writer
                longest = len > longest ? len : longest;
                last_header = i * kTrTile - lead + (long long)(f.first_last >> 16);
            }
        }
    }                                                               // each scan's barrier parts the others' rounds
    longest = (long long)tr_wave_max64((unsigned long long)longest);
    last_header = (long long)tr_wave_max64((unsigned long long)(last_header + 1)) - 1;
    if (lane == 0) { wlen[wave] = longest; wpos[wave] = last_header; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 0; w < kWaves; w++) {
            longest = wlen[w] > longest ? wlen[w] : longest;
            last_header = wpos[w] > last_header ? wpos[w] : last_header;
        }
        const long long headers = carry_h, all = carry_c, upto_last = carry_g;
        const long long e = headers > 0 ? first_e : all;            // candidates that no record holds: the text is malformed
        long long total = 0;
        if (headers > 0) {
            total = (partial ? upto_last : all) - e;
            if (!partial && all - upto_last > longest) longest = all - upto_last;   // the last read ends with the text
        }
        state[kTrN] = partial ? (headers > 0 ? headers - 1 : 0) : headers;
        state[kTrTotal] = total;
        state[kTrLongest] = longest;
        state[kTrConsumed] = !partial ? T : (headers > 0 ? last_header : 0);
        state[kTrBad] = e > 0 ? 0 : -1;
        state[kFaHeaders] = headers;
    }
}

__global__ void __launch_bounds__(kTrBlock) fa_compact_kernel(const uint8_t *__restrict__ text, long long T, int lead, int partial,
                                                              const TrTable table, const long long *__restrict__ last,
                                                              const unsigned long long *__restrict__ cand,
                                                              const unsigned long long *__restrict__ hdrs,
                                                              const long long *__restrict__ state, long long *__restrict__ offs,
                                                              long long *__restrict__ starts, long long cap_reads,
                                                              uint8_t *__restrict__ bases, long long cap_bases)
{
    __shared__ TrTile s;
    __shared__ uint32_t tab[64];
    __shared__ uint4 stage[kTrBlock + 1];                          // the tile's codes, on the 16-byte grid of their address
    const long long n = state[kTrN];
    // block-uniform: the call fails, nothing is stored.  Below, the text is well-formed: its kept bytes are its candidates
    if (state[kTrBad] == 0 || n > cap_reads || state[kTrTotal] > cap_bases) return;
    const int t = threadIdx.x;
    if (t < 64) tab[t] = table.w[t];
    const long long tile = blockIdx.x;
    const int c = tr_load_tile(text, T, lead, tile, s);              // its barriers also cover tab[]
    const long long tile0 = tile * kTrTile - lead;
    const uint8_t *code = reinterpret_cast<const uint8_t *>(tab);
    const TileLane L = fa_classify(text, T, tile0, c, last[tile], partial, state[kTrLastNewline], partial ? state[kTrConsumed] : T, s);
    if (tile == 0 && t == 0) offs[n] = state[kTrTotal];
    // the tile's codes are one run of d_bases, from cand[tile]; header n (GENIE_TEXT_PARTIAL) opens no read of this call
    tile_compact(L, s.wave_total, s.text, stage, (long long)cand[tile], (long long)hdrs[tile], n, bases,
                 [&](long long r, int k, long long at) {
                     offs[r] = at;
                     if (starts) starts[r] = tile0 + 16 * t + k;
                 },
                 [&](uint8_t b) { return code[b]; });
}

struct FastaArea {
    long long *state;
    unsigned long long *cnt;         // per tile (+ 1): FA1
    long long *last;
    unsigned long long *cand, *hdrs; // per tile: FA2, scanned in place
    TileInfo *info;
};

inline int64_t fasta_layout(uint8_t *p, int64_t text_bytes, FastaArea *a)
{
    const int64_t ntiles = tr_tiles(text_bytes, 15);
    Carver c{p};
    c.take(a->state, 8 * kTrStateWords);
    c.take(a->cnt, 8 * (ntiles + 1));
    c.take(a->last, 8 * (ntiles + 1));
    c.take(a->cand, 8 * (ntiles + 1));
    c.take(a->hdrs, 8 * (ntiles + 1));
    c.take(a->info, (int64_t)sizeof(TileInfo) * (ntiles + 1));
    return c.at;
}

}  // namespace

int64_t reads_from_fasta_tmp_bytes(int64_t text_bytes, int64_t cap_reads)
{
    (void)cap_reads;                                                 // nothing is per read
    FastaArea a;
    return fasta_layout(nullptr, text_bytes, &a);
}

int launch_reads_from_fasta(const uint8_t *d_text, int64_t text_bytes, int32_t flags, const uint8_t *code_of_byte, uint8_t *d_bases,
                            int64_t cap_bases, int64_t *d_read_offsets, int64_t *d_record_starts, int64_t cap_reads, int64_t *out5,
                            void *d_tmp, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int partial = (flags & GENIE_TEXT_PARTIAL) ? 1 : 0;
    long long *offs = reinterpret_cast<long long *>(d_read_offsets);
    if (text_bytes == 0) return tr_empty_text(offs, s, out5);
    const int lead = (int)(reinterpret_cast<uintptr_t>(d_text) & 15);
    const long long ntiles = tr_tiles(text_bytes, lead);
    if (ntiles > 0x7fffffffll) return GENIE_E_INVALID;              // one block each
    FastaArea a;
    fasta_layout(static_cast<uint8_t *>(d_tmp), text_bytes, &a);
    const TrTable table = tr_table(code_of_byte);
    const dim3 tblock(kTrBlock);
    dim3 tgrid;
    if (int rc = grid_for(ntiles, kTrBlock, &tgrid)) return rc;
    LAUNCH(tr_count_kernel, tgrid, tblock, 0, s, d_text, (long long)text_bytes, lead, a.cnt, a.last);
    LAUNCH(tr_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, a.cnt, a.last, ntiles, (long long)text_bytes, (int)GENIE_TEXT_LINES, partial,
           a.state);
    LAUNCH(fa_count_kernel, tgrid, tblock, 0, s, d_text, (long long)text_bytes, lead, partial, a.last, a.state, a.cand, a.hdrs, a.info);
    LAUNCH(fa_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, a.cand, a.hdrs, a.info, ntiles, (long long)text_bytes, lead, partial, a.state);
    if (offs)
        LAUNCH(fa_compact_kernel, tgrid, tblock, 0, s, d_text, (long long)text_bytes, lead, partial, table, a.last, a.cand, a.hdrs, a.state,
               offs, reinterpret_cast<long long *>(d_record_starts), (long long)cap_reads, d_bases, (long long)cap_bases);
    long long st[kTrStateWords];
    if (int rc = tr_read_state(a.state, s, st)) return rc;
    out5[0] = st[kTrN];
    out5[1] = st[kTrTotal];
    out5[2] = st[kTrLongest];
    out5[3] = st[kTrConsumed];
    out5[4] = st[kTrBad];
    if (st[kTrBad] == 0) return GENIE_E_INVALID;                    // a non-empty line in front of the first header
    if (offs && (st[kTrN] > cap_reads || st[kTrTotal] > cap_bases)) return GENIE_E_CAPACITY;
    return GENIE_OK;
}

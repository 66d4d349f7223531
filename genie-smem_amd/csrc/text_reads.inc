// text_reads.inc -- genie_reads_from_text: text (one read per line, or four-line FASTQ records) -> base codes back to back
// and int64 offsets, the input of genie_find_smems_long_ex (included by kernels.hip behind ingest_tiles.inc, inside namespace
// genie; uses its launch plumbing, the workspace carver and the block-sums scan).  From ingest_tiles.inc: the tiles and
// their loader, the block scan, tile_stage_store for TR3's second half, and the launch's tail.  Its own: the newline list,
// tr_scan_kernel's two scans, the line lengths and their offsets scan, FASTQ's checks.
//
// Three flat passes over the text, cut into TILES of kTrTile bytes, one block per tile.  Nothing is per read: a line of
// 10^6 bases and 10^5 empty lines cost the same per byte.  Tiles are cut on the 16-byte grid of the text's ADDRESS, not of
// its first byte (the text may start at any address): position i of the text is tile position i + lead, lead = address & 15,
// so every lane's 16 bytes are one aligned load, except the lanes that straddle the text's first or last byte, which load
// byte by byte and never touch memory outside the text.  Every pass starts the same way (tr_load_tile): the tile goes to
// LDS and the positions of its newlines, in order, into a list beside it.
//   TR1 tr_count_kernel    per tile: the number of newlines and the position of the last one (-1: none).
//       tr_scan_kernel     one block: exclusive sum scan and exclusive max scan over the tiles ("newlines before this tile",
//                          "last newline before this tile"), then the call's state: lines, N, consumed bytes.
//   TR2 tr_length_kernel   one thread per newline: the line it ends is line (newlines before it), it starts behind the
//                          previous newline, a '\r' before the newline is dropped.  A sequence line of a complete record
//                          writes its length to d_read_offsets[r + 1]; FASTQ header and plus lines are checked (the first
//                          bad record: a 64-bit atomic minimum).  Per tile the sum of the lengths and their maximum;
//       tr_reduce_kernel   one block adds them up: total_bases and the longest read.
//       tr_offsets_*       the lengths to offsets in place: block sums, scan_block_sums_kernel, inclusive scan per block.
//   TR3 tr_translate_kernel  every lane walks its 16 bytes: the newlines of the tile before them (binary search in the list)
//                          give the line it starts in; a byte of a sequence line inside the line's length is a base.
//                          Reads lie back to back in d_bases, so the bases of a tile are ONE run of it: a block scan of
//                          the lanes' counts places every code (translated through an LDS copy of the table, a kernel
//                          argument) in an LDS image of that run, laid out on the 16-byte grid of its ADDRESS, and the
//                          image is stored 16 bytes per lane, byte by byte only at the run's two ends.
// No atomic decides a position: every output byte and offset is a function of the text alone.  All positions are 64-bit.
namespace {

constexpr unsigned long long kTrNoBad = ~0ull;

struct TrTable {
    uint32_t w[64];                              // code_of_byte, already clamped to 0..4, four entries per word
};

struct TrTile {
    uint4 text[kTrBlock];                        // the tile's bytes (zero outside the text)
    uint16_t nl[kTrTile];                        // tile positions of its newlines, ascending
    uint32_t wave_total[kTrBlock / kWave];
};

// Loads tile `tile` into LDS and lists its newlines; returns their number.  Every thread of the block calls it, once.
__device__ __forceinline__ int tr_load_tile(const uint8_t *__restrict__ text, long long T, int lead, long long tile, TrTile &s)
{
    const int t = threadIdx.x;
    const long long i0 = tile * kTrTile + 16 * t - lead;           // text position of this lane's first byte
    const uint4 w = tile_load_word(text, T, i0, 0u);
    s.text[t] = w;
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
    uint32_t mask = 0;                                              // bit k: byte k of the 16 is a newline
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t z = tr_zero_bytes(ws[j] ^ 0x0A0A0A0Au);
        mask |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * j);
    }
    uint32_t total;
    uint32_t rank = tr_block_exclusive_scan((uint32_t)__popc(mask), s.wave_total, total);
    while (mask) {
        s.nl[rank++] = (uint16_t)(16 * t + __builtin_ctz(mask));
        mask &= mask - 1;
    }
    __syncthreads();
    return (int)total;
}

__device__ __forceinline__ uint8_t tr_tile_byte(const TrTile &s, int q) { return reinterpret_cast<const uint8_t *>(s.text)[q]; }

__global__ void __launch_bounds__(kTrBlock) tr_count_kernel(const uint8_t *__restrict__ text, long long T, int lead,
                                                            unsigned long long *__restrict__ cnt, long long *__restrict__ last)
{
    __shared__ TrTile s;
    const long long tile = blockIdx.x;
    const int c = tr_load_tile(text, T, lead, tile, s);
    if (threadIdx.x == 0) {
        cnt[tile] = (unsigned long long)c;
        last[tile] = c ? tile * kTrTile + s.nl[c - 1] - lead : -1ll;
    }
}

// single block: cnt[] -> newlines before each tile, last[] -> last newline before each tile (-1: none); then the state
// (its two scans share one barrier and one pass over the waves' totals; through tile_scan64, one scan behind the other, the
// call measured 10 to 30 us slower on 150 to 300 MB of text, so they stay written out)
__global__ void __launch_bounds__(kScanBlock) tr_scan_kernel(unsigned long long *__restrict__ cnt, long long *__restrict__ last,
                                                             long long ntiles, long long T, int format, int partial,
                                                             long long *__restrict__ state)
{
    __shared__ unsigned long long wsum[kScanBlock / kWave];
    __shared__ long long wmax[kScanBlock / kWave];
    __shared__ unsigned long long carry_sum;
    __shared__ long long carry_max;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) { carry_sum = 0; carry_max = -1; }
    __syncthreads();
    for (long long base = 0; base < ntiles; base += kScanBlock) {
        const long long i = base + threadIdx.x;
        const unsigned long long c = i < ntiles ? cnt[i] : 0ull;
        const long long l = i < ntiles ? last[i] : -1ll;
        const unsigned long long inc = wave_inclusive_scan64(c, lane);
        long long mx = l;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const long long v = tr_shfl_up64(mx, off);
            if (lane >= off && v > mx) mx = v;
        }
        if (lane == kWave - 1) { wsum[wave] = inc; wmax[wave] = mx; }
        long long ex = tr_shfl_up64(mx, 1);                         // exclusive within the wave
        if (lane == 0) ex = -1;
        __syncthreads();
        unsigned long long before = carry_sum, all = 0;
        long long mbefore = carry_max, mall = carry_max;
        for (int w = 0; w < kScanBlock / kWave; w++) {
            const unsigned long long x = wsum[w];
            const long long y = wmax[w];
            before += w < wave ? x : 0ull;
            all += x;
            if (w < wave && y > mbefore) mbefore = y;
            if (y > mall) mall = y;
        }
        if (i < ntiles) {
            cnt[i] = before + inc - c;
            last[i] = ex > mbefore ? ex : mbefore;
        }
        __syncthreads();
        if (threadIdx.x == 0) { carry_sum += all; carry_max = mall; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const long long newlines = (long long)carry_sum, last_nl = carry_max;
        const bool tail_line = !partial && last_nl + 1 < T;
        const long long lines = newlines + (tail_line ? 1 : 0);
        const long long n = format == GENIE_TEXT_FASTQ ? lines / 4 : lines;
        state[kTrN] = n;
        // with GENIE_TEXT_PARTIAL: where the first unconsumed line starts (FASTQ: TR2 writes the start of line 4N when N > 0)
        state[kTrConsumed] = !partial ? T : (format == GENIE_TEXT_FASTQ ? 0 : last_nl + 1);
        state[kTrBad] = (long long)kTrNoBad;
        state[kTrLines] = lines;
        state[kTrNewlines] = newlines;
        state[kTrLastNewline] = last_nl;
    }
}

// offs: d_read_offsets or null (the sizing call); lengths go to offs[r + 1] for r < cap_reads
__global__ void __launch_bounds__(kTrBlock) tr_length_kernel(const uint8_t *__restrict__ text, long long T, int lead, int format,
                                                             int partial, const unsigned long long *__restrict__ cnt,
                                                             const long long *__restrict__ last, long long *__restrict__ state,
                                                             long long *__restrict__ offs, long long cap_reads,
                                                             unsigned long long *__restrict__ tile_sum,
                                                             unsigned long long *__restrict__ tile_max)
{
    __shared__ TrTile s;
    __shared__ unsigned long long part[2][kTrBlock / kWave];
    const long long tile = blockIdx.x;
    const int c = tr_load_tile(text, T, lead, tile, s);
    const long long tile0 = tile * kTrTile - lead;                  // text position of tile position 0
    const long long line0 = (long long)cnt[tile], prev0 = last[tile];
    const long long n = state[kTrN];
    auto byte_at = [&](long long i) -> uint8_t {
        const long long q = i - tile0;
        return q >= 0 && q < kTrTile ? tr_tile_byte(s, (int)q) : text[i];
    };
    unsigned long long sum = 0, longest = 0;
    auto read_length = [&](long long r, long long len) {
        if (offs && r < cap_reads) offs[r + 1] = len;
        sum += (unsigned long long)len;
        longest = (unsigned long long)len > longest ? (unsigned long long)len : longest;
    };
    for (int m = threadIdx.x; m < c; m += kTrBlock) {
        const long long i = tile0 + s.nl[m];
        const long long prev = m > 0 ? tile0 + s.nl[m - 1] : prev0;
        const long long j = line0 + m;                              // the line this newline ends
        long long len = i - prev - 1;
        if (len > 0 && byte_at(i - 1) == '\r') len--;
        if (format == GENIE_TEXT_LINES) {
            read_length(j, len);
        } else {
            const long long r = j >> 2;
            const int k = (int)(j & 3);
            if (r < n) {
                if (k == 1) read_length(r, len);
                else if (k == 0 || k == 2) {
                    if (len <= 0 || byte_at(prev + 1) != (k == 0 ? '@' : '+'))
                        atomicMin(reinterpret_cast<unsigned long long *>(state + kTrBad), (unsigned long long)r);
                } else if (partial && r == n - 1) {
                    state[kTrConsumed] = i + 1;                      // the start of line 4N: one writer
                }
            }
        }
    }
    // the bytes behind the last newline are one more line (no '\r' is dropped); in FASTQ that line is never a sequence
    // line of a complete record
    if (tile == 0 && threadIdx.x == 0 && !partial && format == GENIE_TEXT_LINES) {
        const long long last_nl = state[kTrLastNewline];
        if (last_nl + 1 < T) read_length(state[kTrNewlines], T - last_nl - 1);
    }
    // the tile's share of total_bases and of the longest read: one pair per tile, summed up by tr_reduce_kernel (a hundred
    // thousand atomics on one address would take longer than the three passes)
    sum = wave_sum64(sum);
    longest = tr_wave_max64(longest);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        part[0][threadIdx.x >> 6] = sum;
        part[1][threadIdx.x >> 6] = longest;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long a = 0, b = 0;
        for (int w = 0; w < kTrBlock / kWave; w++) {
            a += part[0][w];
            b = part[1][w] > b ? part[1][w] : b;
        }
        tile_sum[tile] = a;
        tile_max[tile] = b;
    }
}

// single block: the tiles' sums and maxima -> total_bases and the longest read
__global__ void __launch_bounds__(kScanBlock) tr_reduce_kernel(const unsigned long long *__restrict__ tile_sum,
                                                               const unsigned long long *__restrict__ tile_max, long long ntiles,
                                                               long long *__restrict__ state)
{
    __shared__ unsigned long long part[2][kScanBlock / kWave];
    unsigned long long a = 0, b = 0;
    for (long long i = threadIdx.x; i < ntiles; i += kScanBlock) {
        a += tile_sum[i];
        const unsigned long long x = tile_max[i];
        b = x > b ? x : b;
    }
    a = wave_sum64(a);
    b = tr_wave_max64(b);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        part[0][threadIdx.x >> 6] = a;
        part[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = 0;
        for (int w = 0; w < kScanBlock / kWave; w++) {
            a += part[0][w];
            b = part[1][w] > b ? part[1][w] : b;
        }
        state[kTrTotal] = (long long)a;
        state[kTrLongest] = (long long)b;
    }
}

// lengths at offs[1 .. N] -> offsets, in place.  Nothing is done when the reads do not fit (the call fails).
__global__ void __launch_bounds__(kScanBlock) tr_offsets_block_sums(const long long *__restrict__ offs, const long long *__restrict__ state,
                                                                    long long cap_reads, unsigned long long *__restrict__ block_sums)
{
    __shared__ unsigned long long wsum[kScanBlock / kWave];
    const long long n = state[kTrN];
    const long long i = (long long)blockIdx.x * kScanBlock + threadIdx.x;
    unsigned long long v = n <= cap_reads && i < n ? (unsigned long long)offs[i + 1] : 0ull;
    v = wave_sum64(v);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kScanBlock / kWave; w++) t += wsum[w];
        block_sums[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(kScanBlock) tr_offsets_apply(long long *__restrict__ offs, const long long *__restrict__ state,
                                                               long long cap_reads, const unsigned long long *__restrict__ block_sums)
{
    __shared__ unsigned long long wave_total[kScanBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const long long n = state[kTrN];
    const long long i = (long long)blockIdx.x * kScanBlock + threadIdx.x;
    const bool mine = n <= cap_reads && i < n;
    const unsigned long long v = mine ? (unsigned long long)offs[i + 1] : 0ull;
    const unsigned long long inc = wave_inclusive_scan64(v, lane);
    if (lane == kWave - 1) wave_total[wave] = inc;
    __syncthreads();
    unsigned long long base = block_sums[blockIdx.x] + inc;
    for (int w = 0; w < wave; w++) base += wave_total[w];
    if (mine) offs[i + 1] = (long long)base;
    if (i == 0) offs[0] = 0;
}

__global__ void __launch_bounds__(kTrBlock) tr_translate_kernel(const uint8_t *__restrict__ text, long long T, int lead, int format,
                                                                const TrTable table, const unsigned long long *__restrict__ cnt,
                                                                const long long *__restrict__ last, const long long *__restrict__ state,
                                                                const long long *__restrict__ offs, long long cap_reads,
                                                                uint8_t *__restrict__ bases, long long cap_bases)
{
    __shared__ TrTile s;
    __shared__ uint32_t tab[64];
    __shared__ uint4 stage[kTrBlock + 1];                          // the tile's codes, on the 16-byte grid of their address
    __shared__ long long first_dst;
    const long long n = state[kTrN];
    if (n > cap_reads || state[kTrTotal] > cap_bases) return;      // block-uniform: the call fails, nothing is stored
    const int t = threadIdx.x;
    if (t < 64) tab[t] = table.w[t];
    const long long tile = blockIdx.x;
    const int c = tr_load_tile(text, T, lead, tile, s);              // its barriers also cover tab[]
    const long long tile0 = tile * kTrTile - lead;
    const long long line0 = (long long)cnt[tile], prev0 = last[tile];
    const uint8_t *code = reinterpret_cast<const uint8_t *>(tab);
    // this lane's 16 bytes, in text order: which of them are bases of a read, and where the first of those goes
    int m = 0, hi = c;                                              // m = newlines of the tile before the lane's first byte
    while (m < hi) {
        const int mid = (m + hi) >> 1;
        if (s.nl[mid] < 16 * t) m = mid + 1; else hi = mid;
    }
    long long start = (m > 0 ? tile0 + s.nl[m - 1] : prev0) + 1;    // of the line the next byte belongs to
    const long long i0 = tile0 + 16 * t;
    const uint4 w = s.text[t];
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
    bool fresh = true, seq = false;
    long long o0 = 0, len = 0, dst = 0;
    uint32_t keep = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const long long i = i0 + k;
        if (i < 0 || i >= T) continue;
        if (((ws[k >> 2] >> (8 * (k & 3))) & 0xFFu) == '\n') {
            m++;
            start = i + 1;
            fresh = true;
            continue;
        }
        if (fresh) {
            fresh = false;
            const long long j = line0 + m;
            const long long r = format == GENIE_TEXT_FASTQ ? j >> 2 : j;
            // not the tail of a partial text, not a line of an incomplete record
            seq = (format != GENIE_TEXT_FASTQ || (j & 3) == 1) && r < n;
            if (seq) {
                o0 = offs[r];
                len = offs[r + 1] - o0;
            }
        }
        if (seq && i - start < len) {                                // not the '\r' that the line's length leaves out
            if (!keep) dst = o0 + (i - start);
            keep |= 1u << k;
        }
    }
    // The bases of consecutive reads lie back to back, so the tile's codes are one run of d_bases: it starts where the
    // first lane that keeps a byte puts it, and a lane's codes follow those of the lanes before it.
    uint32_t total;
    const uint32_t before = tr_block_exclusive_scan((uint32_t)__popc(keep), s.wave_total, total);
    if (keep && before == 0) first_dst = dst;
    __syncthreads();
    tile_stage_store(keep, before, total, s.text, stage, bases, first_dst, [&](uint8_t b) { return code[b]; });
}

inline int64_t tr_scan_blocks(int64_t text_bytes, int64_t cap_reads)
{
    const int64_t most = cap_reads < text_bytes ? cap_reads : text_bytes;   // a text of T bytes has at most T lines
    return most < 1 ? 1 : (most + kScanBlock - 1) / kScanBlock;
}

// code_of_byte as it travels to the kernels: clamped to 0..4
inline TrTable tr_table(const uint8_t *code_of_byte)
{
    TrTable table;
    for (int i = 0; i < 64; i++) {
        uint32_t w = 0;
        for (int k = 0; k < 4; k++) {
            const uint8_t c = code_of_byte[4 * i + k];
            w |= (uint32_t)(c <= 3 ? c : 4) << (8 * k);
        }
        table.w[i] = w;
    }
    return table;
}

struct TextArea {
    long long *state;
    unsigned long long *cnt;         // per tile (+ 1)
    long long *last;
    unsigned long long *tile_sum, *tile_max;   // per tile: the bases of its lines, the longest of them
    unsigned long long *sums;        // block sums of the offsets scan (+ 1: the grand total)
};

inline int64_t text_layout(uint8_t *p, int64_t text_bytes, int64_t cap_reads, TextArea *a)
{
    const int64_t ntiles = tr_tiles(text_bytes, 15);
    Carver c{p};
    c.take(a->state, 8 * kTrStateWords);
    c.take(a->cnt, 8 * (ntiles + 1));
    c.take(a->last, 8 * (ntiles + 1));
    c.take(a->tile_sum, 8 * (ntiles + 1));
    c.take(a->tile_max, 8 * (ntiles + 1));
    c.take(a->sums, 8 * (tr_scan_blocks(text_bytes, cap_reads) + 1));
    return c.at;
}

}  // namespace

int64_t reads_from_text_tmp_bytes(int64_t text_bytes, int64_t cap_reads)
{
    TextArea a;
    return text_layout(nullptr, text_bytes, cap_reads, &a);
}

int launch_reads_from_text(const uint8_t *d_text, int64_t text_bytes, int32_t format, int32_t flags, const uint8_t *code_of_byte,
                           uint8_t *d_bases, int64_t cap_bases, int64_t *d_read_offsets, int64_t cap_reads, int64_t *out5,
                           void *d_tmp, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int partial = (flags & GENIE_TEXT_PARTIAL) ? 1 : 0;
    long long *offs = reinterpret_cast<long long *>(d_read_offsets);
    if (text_bytes == 0) return tr_empty_text(offs, s, out5);
    const int lead = (int)(reinterpret_cast<uintptr_t>(d_text) & 15);
    const long long ntiles = tr_tiles(text_bytes, lead);
    if (ntiles > 0x7fffffffll || tr_scan_blocks(text_bytes, cap_reads) > 0x7fffffffll) return GENIE_E_INVALID;   // one block each
    TextArea a;
    text_layout(static_cast<uint8_t *>(d_tmp), text_bytes, cap_reads, &a);
    const TrTable table = tr_table(code_of_byte);
    const dim3 tblock(kTrBlock);
    dim3 tgrid;
    if (int rc = grid_for(ntiles, kTrBlock, &tgrid)) return rc;
    LAUNCH(tr_count_kernel, tgrid, tblock, 0, s, d_text, (long long)text_bytes, lead, a.cnt, a.last);
    LAUNCH(tr_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, a.cnt, a.last, ntiles, (long long)text_bytes, (int)format, partial, a.state);
    LAUNCH(tr_length_kernel, tgrid, tblock, 0, s, d_text, (long long)text_bytes, lead, (int)format, partial, a.cnt, a.last, a.state, offs,
           (long long)cap_reads, a.tile_sum, a.tile_max);
    LAUNCH(tr_reduce_kernel, dim3(1), dim3(kScanBlock), 0, s, a.tile_sum, a.tile_max, ntiles, a.state);
    if (offs) {
        const long long nblocks = tr_scan_blocks(text_bytes, cap_reads);
        LAUNCH_BLOCKS(tr_offsets_block_sums, nblocks, kScanBlock, 0, s, offs, a.state, (long long)cap_reads, a.sums);
        LAUNCH(scan_block_sums_kernel, dim3(1), dim3(kScanBlock), 0, s, a.sums, nblocks);
        LAUNCH_BLOCKS(tr_offsets_apply, nblocks, kScanBlock, 0, s, offs, a.state, (long long)cap_reads, a.sums);
        LAUNCH(tr_translate_kernel, tgrid, tblock, 0, s, d_text, (long long)text_bytes, lead, (int)format, table, a.cnt, a.last, a.state,
               offs, (long long)cap_reads, d_bases, (long long)cap_bases);
    }
    long long st[kTrStateWords];
    if (int rc = tr_read_state(a.state, s, st)) return rc;
    out5[0] = st[kTrN];
    out5[1] = st[kTrTotal];
    out5[2] = st[kTrLongest];
    out5[3] = st[kTrConsumed];
    out5[4] = -1;
    if ((unsigned long long)st[kTrBad] != kTrNoBad) {
        out5[4] = st[kTrBad];
        return GENIE_E_INVALID;
    }
    if (format == GENIE_TEXT_FASTQ && !partial && (st[kTrLines] & 3) != 0) {
        out5[4] = st[kTrN];                                          // the first incomplete record
        return GENIE_E_INVALID;
    }
    if (offs && (st[kTrN] > cap_reads || st[kTrTotal] > cap_bases)) return GENIE_E_CAPACITY;
    return GENIE_OK;
}

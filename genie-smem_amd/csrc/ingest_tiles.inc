// ingest_tiles.inc -- what the three ingestion calls share: genie_reads_from_text (text_reads.inc), genie_reads_from_fasta
// (fasta_reads.inc) and genie_reference_segments (segments.inc).  Included by kernels.hip in front of them, inside
// namespace genie; the helpers are for these three files only.
//
// All three read their input in TILES of kTrTile bytes, one block per tile, cut on the 16-byte grid of the input's ADDRESS:
// position i of the input is tile position i + lead, lead = address & 15, so every lane's 16 bytes are one aligned load
// (tile_load_word).  A lane classifies its 16 bytes into two masks, a TileLane: the bytes the call KEEPS and the MARKS
// among them (FASTA: a header's '>', which is not kept; segments: a segment's first base).  The output is the stream
// compaction of the kept bytes, and a mark's offset is the number of kept bytes in front of it:
//   tile_count     per tile: kept bytes and marks, the kept bytes in front of its first and of its last mark, the most
//                  kept bytes between two of its marks, where its first and last mark lie (a TileInfo).
//   tile_scan64    one block over the tiles: an exclusive 64-bit sum or maximum of kScanBlock values on top of a carry.
//   tile_compact   per tile: every mark goes to the caller's writer with its index and offset; then tile_stage_store
//                  places every kept byte's code in an LDS image of the tile's run of the output, laid out on the 16-byte
//                  grid of its ADDRESS, and tr_store_run stores it 16 bytes per lane, byte by byte only at its two ends.
// On the host, tr_read_state ends every launch and tr_empty_text is the two text calls' answer to an empty text.
namespace {

constexpr int kTrBlock = 256;
constexpr int kTrTile = 16 * kTrBlock;           // bytes of input per block: 16 per lane
// Marks per tile, the one bound of tile_count's list: every byte of a tile of segments can be a start.  FASTA stays below
// it: a header needs a '\n' in front of it (or the text's start), kTrTile / 2 + 1 at the most.
constexpr int kTileMaxMarks = kTrTile;

// the call's state, in the workspace (int64 each); the host copies it back at the end of the call
enum { kTrN = 0, kTrTotal, kTrLongest, kTrConsumed, kTrBad, kTrLines, kTrNewlines, kTrLastNewline, kTrStateWords };

struct TileLane {
    uint32_t keep, mark;                         // bit k: byte k of the lane's 16 is kept / is a mark
};

// what tile_count leaves per tile beside the two counts
struct TileInfo {
    uint32_t first_last;     // tile position of the first mark | of the last mark << 16 (tiles with marks only)
    uint32_t before_first;   // kept bytes of the tile in front of its first mark
    uint32_t before_last;    // ... in front of its last mark
    uint32_t longest;        // the most kept bytes between two consecutive marks of the tile
};

// tile_count's LDS
struct TileMarks {
    uint16_t before[kTileMaxMarks];              // per mark of the tile: the tile's kept bytes in front of it
    uint16_t first, last;                        // tile positions of its first and of its last mark
    uint32_t part[kTrBlock / kWave];
};

// 0x80 in every byte of x that is zero (exact: no carry between bytes)
__device__ __forceinline__ uint32_t tr_zero_bytes(uint32_t x)
{
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// Exclusive scan of one count per thread over the block, and the block's total.  Every thread calls it; a barrier lies
// between two calls that share `wave_total`.
__device__ __forceinline__ uint32_t tr_block_exclusive_scan(uint32_t c, uint32_t *wave_total, uint32_t &total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    uint32_t inc = c;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, off, kWave);
        if (lane >= off) inc += v;
    }
    if (lane == kWave - 1) wave_total[wave] = inc;
    __syncthreads();
    uint32_t before = inc - c;
    total = 0;
#pragma unroll
    for (int wv = 0; wv < kTrBlock / kWave; wv++) {
        const uint32_t x = wave_total[wv];
        before += wv < wave ? x : 0u;
        total += x;
    }
    return before;
}

// The 16 bytes of the input [0, T) from position i0 on, i0 a multiple of 16 off the input's address: one aligned load when
// they lie inside, byte by byte at the input's two ends (never touching memory outside it), `fill` in every byte outside.
__device__ __forceinline__ uint4 tile_load_word(const uint8_t *__restrict__ text, long long T, long long i0, uint32_t fill)
{
    const uint32_t f = fill * 0x01010101u;
    uint4 w = make_uint4(f, f, f, f);
    if (i0 >= 0 && i0 + 16 <= T) {
        w = *reinterpret_cast<const uint4 *>(text + i0);
    } else if (i0 + 16 > 0 && i0 < T) {
        uint32_t x[4] = {f, f, f, f};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const long long i = i0 + k;
            if (i >= 0 && i < T) x[k >> 2] ^= (uint32_t)(uint8_t)(text[i] ^ fill) << (8 * (k & 3));
        }
        w = make_uint4(x[0], x[1], x[2], x[3]);
    }
    return w;
}

// The count pass behind the classifier.  Every thread of the block calls it, once; `wave_total` as in tr_block_exclusive_scan.
__device__ __forceinline__ void tile_count(const TileLane L, uint32_t *wave_total, TileMarks &m, long long tile,
                                           unsigned long long *__restrict__ kept, unsigned long long *__restrict__ marks,
                                           TileInfo *__restrict__ info)
{
    const int t = threadIdx.x;
    uint32_t total;                                                 // kept bytes in the low half, marks in the high half
    const uint32_t before = tr_block_exclusive_scan((uint32_t)__popc(L.keep) | ((uint32_t)__popc(L.mark) << 16), wave_total, total);
    const int nh = (int)(total >> 16);
    int h = (int)(before >> 16);
    uint32_t rest = L.mark;
    while (rest) {
        const int k = __builtin_ctz(rest);
        if (h == 0) m.first = (uint16_t)(16 * t + k);
        if (h == nh - 1) m.last = (uint16_t)(16 * t + k);
        m.before[h++] = (uint16_t)((before & 0xFFFFu) + __popc(L.keep & ((1u << k) - 1u)));
        rest &= rest - 1;
    }
    __syncthreads();
    uint32_t longest = 0;
    for (int i = t + 1; i < nh; i += kTrBlock) {
        const uint32_t len = (uint32_t)m.before[i] - (uint32_t)m.before[i - 1];
        longest = len > longest ? len : longest;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t x = (uint32_t)__shfl_xor((int)longest, off, kWave);
        longest = x > longest ? x : longest;
    }
    if ((t & (kWave - 1)) == 0) m.part[t >> 6] = longest;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kTrBlock / kWave; w++) longest = m.part[w] > longest ? m.part[w] : longest;
        kept[tile] = total & 0xFFFFu;
        marks[tile] = (unsigned long long)nh;
        TileInfo f = {0u, 0u, 0u, 0u};
        if (nh > 0) {
            f.first_last = (uint32_t)m.first | ((uint32_t)m.last << 16);
            f.before_first = m.before[0];
            f.before_last = m.before[nh - 1];
            f.longest = longest;
        }
        info[tile] = f;
    }
}

__device__ __forceinline__ long long tr_shfl_up64(long long v, int off)
{
    const unsigned int lo = (unsigned)__shfl_up((int)(unsigned)(unsigned long long)v, off, kWave);
    const unsigned int hi = (unsigned)__shfl_up((int)(unsigned)((unsigned long long)v >> 32), off, kWave);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ unsigned long long tr_wave_max64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int lo = (unsigned)__shfl_xor((int)(unsigned)v, off, kWave);
        const unsigned int hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off, kWave);
        const unsigned long long x = ((unsigned long long)hi << 32) | lo;
        v = x > v ? x : v;
    }
    return v;
}

// One step of a scan carried over the tiles, kScanBlock at a time: what lies in front of this thread's v -- `carry` and
// the v of the threads before it, added up (kMax: the largest of them).  `carry` becomes that of the whole block, in every
// thread.  Every thread of a kScanBlock block calls it; w: kScanBlock / kWave words of LDS, and a barrier lies between two
// calls that share them.
template <bool kMax>
__device__ __forceinline__ long long tile_scan64(long long v, long long &carry, long long *w)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    auto join = [](long long a, long long b) { return kMax ? (b > a ? b : a) : a + b; };
    long long inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const long long x = tr_shfl_up64(inc, off);
        if (lane >= off) inc = join(inc, x);
    }
    if (lane == kWave - 1) w[wave] = inc;
    const long long up = tr_shfl_up64(inc, 1);                      // exclusive within the wave
    long long ex = lane == 0 ? carry : join(carry, up);
    __syncthreads();
#pragma unroll 4
    for (int wv = 0; wv < kScanBlock / kWave; wv++) {
        const long long y = w[wv];
        if (wv < wave) ex = join(ex, y);
        carry = join(carry, y);
    }
    return ex;
}

// The block's run of codes, staged in LDS on the 16-byte grid of its destination: stage bytes [olead, olead + total) go to
// bases[d0 .. d0 + total), 16 bytes per lane, byte by byte only at the run's two ends.  Every thread of the block calls it,
// behind the barrier that follows the staging.
__device__ __forceinline__ void tr_store_run(const uint4 *stage, int olead, int total, uint8_t *__restrict__ bases, long long d0)
{
    const uint8_t *st = reinterpret_cast<const uint8_t *>(stage);
    const int end = olead + total;
    for (int ch = threadIdx.x; 16 * ch < end; ch += kTrBlock) {
        const int lo = 16 * ch;
        if (lo >= olead && lo + 16 <= end) {
            *reinterpret_cast<uint4 *>(bases + (d0 + (lo - olead))) = stage[ch];
        } else {
            for (int k = 0; k < 16; k++)
                if (lo + k >= olead && lo + k < end) bases[d0 + (lo + k - olead)] = st[lo + k];
        }
    }
}

// The tile's kept bytes are ONE run of the output, bases[d0 .. d0 + total): this lane's follow the `before` of the lanes in
// front of it.  code_of(byte) of each goes to `stage` (kTrBlock + 1 words of LDS), and the run is stored.  `text`: the tile
// in LDS.  Every thread of the block calls it; total is block-uniform.
template <class Code>
__device__ __forceinline__ void tile_stage_store(uint32_t keep, uint32_t before, uint32_t total, const uint4 *text, uint4 *stage,
                                                 uint8_t *__restrict__ bases, long long d0, Code code_of)
{
    if (total == 0) return;
    const int olead = (int)(reinterpret_cast<uintptr_t>(bases + d0) & 15);
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(text);
    uint8_t *st = reinterpret_cast<uint8_t *>(stage);
    int at = olead + (int)before;
    while (keep) {
        st[at++] = code_of(tb[16 * threadIdx.x + __builtin_ctz(keep)]);
        keep &= keep - 1;
    }
    __syncthreads();
    tr_store_run(stage, olead, (int)total, bases, d0);
}

// The compact pass behind the classifier: d0 and mark0 are the kept bytes and the marks in front of the tile.  Mark r < n of
// the tile, byte k of this lane's 16, `at` kept bytes in front of it in the whole input: on_mark(r, k, at), called by the
// lane that holds it.  Then the kept bytes, as tile_stage_store has it.  Every thread of the block calls it, once.
template <class Mark, class Code>
__device__ __forceinline__ void tile_compact(const TileLane L, uint32_t *wave_total, const uint4 *text, uint4 *stage, long long d0,
                                             long long mark0, long long n, uint8_t *__restrict__ bases, Mark on_mark, Code code_of)
{
    uint32_t total;
    const uint32_t before = tr_block_exclusive_scan((uint32_t)__popc(L.keep) | ((uint32_t)__popc(L.mark) << 16), wave_total, total);
    long long r = mark0 + (before >> 16);
    uint32_t rest = L.mark;
    while (rest && r < n) {
        const int k = __builtin_ctz(rest);
        on_mark(r++, k, d0 + (before & 0xFFFFu) + __popc(L.keep & ((1u << k) - 1u)));
        rest &= rest - 1;
    }
    tile_stage_store(L.keep, before & 0xFFFFu, total & 0xFFFFu, text, stage, bases, d0, code_of);
}

inline long long tr_tiles(int64_t text_bytes, int lead) { return (text_bytes + lead + kTrTile - 1) / kTrTile; }

// The tail of a launch: the call's state in st[kTrStateWords], behind everything the stream held.  Each call maps it to
// its own out[] and status.
inline int tr_read_state(const long long *d_state, hipStream_t s, long long *st)
{
    HIP_TRY(hipMemcpyAsync(st, d_state, 8 * kTrStateWords, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GENIE_OK;
}

// what the two text calls answer to an empty text: no read, nothing consumed, d_read_offsets[0] = 0 when it is given
inline int tr_empty_text(long long *offs, hipStream_t s, int64_t *out5)
{
    if (offs) HIP_TRY(hipMemsetAsync(offs, 0, 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    out5[0] = out5[1] = out5[2] = out5[3] = 0;
    out5[4] = -1;
    return GENIE_OK;
}

}  // namespace

// segments.inc -- genie_reference_segments and genie_segment_coords: a reference with ambiguous bases is cut at its breaks
// (codes > 3) and at its record boundaries into SEGMENTS, the maximal runs of A/C/G/T inside one record (included by
// kernels.hip behind contigs.inc and fasta_reads.inc, inside namespace genie; uses the tile scan of fasta_reads.inc and
// the table lookup of contigs.inc).  From ingest_tiles.inc: the loader (fill 0xFF, a break), tile_count and tile_compact
// behind the classifier, the launch's tail.  Its own: sg_load_tile's boundary bitmap and classification, the error mask
// in front of both passes, and the writer of a start's offset, record and origin.
//
// d_bases is the STREAM COMPACTION of the kept bytes and d_seg_offsets[s] the kept bytes in front of segment s: the shape of
// genie_reads_from_fasta with "kept byte" for candidate and "segment start" for header.  A kept byte is a START when the byte
// in front of it is a break, when it is the first of the reference, or when a record boundary lies on it.  Two reads of the
// given codes, in tiles of kTrTile bytes on the 16-byte grid of their address, one block per tile:
//   SG0 ctg_validate_kernel (contigs.inc)  the record table's three conditions -> the error mask.  A bad table ends the call:
//                          the passes below see the mask and store nothing (SG1: zeros for its tile).
//   SG1 sg_count_kernel    tile_count.  Per tile: kept bytes and starts; the kept bytes in front of its first and of its
//                          last start; the most kept bytes between two of its starts.
//       fa_scan_kernel (fasta_reads.inc)   exclusive sums of both counts; its exclusive maximum of "kept bytes in front of the
//                          last start so far" closes the segments that cross tiles: n_seg, n_kept and the longest segment.
//   SG2 sg_compact_kernel  tile_compact: places every kept code in an LDS image of the tile's run of d_bases and stores it
//                          coalesced; the lane that holds a start writes the segment's offset, record and origin.
// Record boundaries cost nothing per byte (sg_boundaries): two lanes bisect the table for the tile's first byte and for
// the byte behind its last, the block sets one bit per boundary between them in an LDS bitmap of the tile (equal
// offsets, the empty records, collapse: an entry equal to the one in front of it is skipped), and every lane reads its 16
// bits.  A start's record is the last r with off[r] <= i: a bisection of those same entries, which are none in most tiles.
// The only atomics are the ORs of the error mask and of the bitmap: no output depends on an order.  Positions are 64-bit.
namespace {

enum { kSgMask = kTrNewlines };                  // the state word fa_scan_kernel leaves alone: the table's error mask

struct SgTile {
    uint4 text[kTrBlock];                        // the tile's codes (0xFF, a break, outside the reference)
    uint32_t bnd[kTrTile / 32];                  // bit q: a record boundary lies on tile position q
    long long range[2];                          // the table entries with a value inside the tile are [range[0], range[1])
    uint32_t wave_total[kTrBlock / kWave];
};

// The first index in [0, nrec + 1] whose entry is not below `key` (nrec + 1: none).  Moves inside the table whatever it holds.
__device__ __forceinline__ long long sg_lower_bound(const long long *__restrict__ off, long long nrec, long long key)
{
    long long lo = 0, hi = nrec + 1;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (off[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The record of given position i, the last r with off[r] <= i (ctg_find's rule in 64 bits; empty records own nothing),
// among the entries [lo, hi) that lie inside i's tile; clamped into [0, nrec - 1].
__device__ __forceinline__ long long sg_record_of(const long long *__restrict__ off, long long nrec, long long lo, long long hi, long long i)
{
    while (lo < hi) {                                               // every entry in front of lo is <= i
        const long long mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= i) lo = mid + 1; else hi = mid;
    }
    const long long r = lo - 1;
    return r < 0 ? 0 : (r > nrec - 1 ? nrec - 1 : r);
}

// Loads the tile, stages its record boundaries and classifies this lane's 16 bytes.  Every thread of the block calls it, once;
// the tile and s.range are readable behind it.
__device__ __forceinline__ TileLane sg_load_tile(const uint8_t *__restrict__ codes, long long n, int lead, long long tile,
                                                 const long long *__restrict__ off, long long nrec, SgTile &s)
{
    const int t = threadIdx.x;
    const long long tile0 = tile * kTrTile - lead;                  // given position of tile position 0
    const long long i0 = tile0 + 16 * t;
    const uint4 w = tile_load_word(codes, n, i0, 0xFFu);
    s.text[t] = w;
    if (t < kTrTile / 32) s.bnd[t] = 0u;
    if (off && t < 2) {                                             // lane 0: the first byte's entries; lane 1: behind the last byte
        const long long first = tile0 < 0 ? 0 : tile0;
        s.range[t] = sg_lower_bound(off, nrec, t == 0 ? first : tile0 + kTrTile);
    }
    __syncthreads();
    if (off) {
        const long long lo = s.range[0], hi = s.range[1];
        for (long long r = lo + t; r < hi; r += kTrBlock) {
            const long long v = off[r], q = v - tile0;
            if (q >= 0 && q < kTrTile && v < n && (r == lo || off[r - 1] != v)) atomicOr(&s.bnd[q >> 5], 1u << (q & 31));
        }
        __syncthreads();
    }
    const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
    TileLane L = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; j++) {                                   // a code is kept when it is at most 3: its upper six bits are 0
        const uint32_t z = tr_zero_bytes(ws[j] & 0xFCFCFCFCu);
        L.keep |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * j);
    }
    uint32_t prev = 0xFFu;                                          // the byte in front of the lane's first
    if (t > 0) prev = reinterpret_cast<const uint8_t *>(s.text)[16 * t - 1];
    else if (tile0 > 0 && tile0 - 1 < n) prev = codes[tile0 - 1];
    const uint32_t before = (L.keep << 1) | (prev <= 3u ? 1u : 0u); // bit k: the byte in front of byte k is kept
    const uint32_t bnd = (s.bnd[t >> 1] >> (16 * (t & 1))) & 0xFFFFu;
    L.mark = L.keep & (~before | bnd) & 0xFFFFu;
    return L;
}

__global__ void __launch_bounds__(kTrBlock) sg_count_kernel(const uint8_t *__restrict__ codes, long long n, int lead,
                                                            const long long *__restrict__ off, long long nrec,
                                                            const long long *__restrict__ state, unsigned long long *__restrict__ kept,
                                                            unsigned long long *__restrict__ starts, TileInfo *__restrict__ info)
{
    __shared__ SgTile s;
    __shared__ TileMarks m;
    const long long tile = blockIdx.x;
    if (state[kSgMask] != 0) {                                      // block-uniform: a bad table, the call fails
        if (threadIdx.x == 0) {
            kept[tile] = starts[tile] = 0ull;
            info[tile] = TileInfo{0u, 0u, 0u, 0u};
        }
        return;
    }
    tile_count(sg_load_tile(codes, n, lead, tile, off, nrec, s), s.wave_total, m, tile, kept, starts, info);
}

__global__ void __launch_bounds__(kTrBlock) sg_compact_kernel(const uint8_t *__restrict__ codes, long long n, int lead,
                                                              const long long *__restrict__ off, long long nrec,
                                                              const long long *__restrict__ state,
                                                              const unsigned long long *__restrict__ kept,
                                                              const unsigned long long *__restrict__ starts, uint8_t *__restrict__ bases,
                                                              long long cap_bases, long long *__restrict__ seg_off,
                                                              int32_t *__restrict__ seg_rec, long long *__restrict__ seg_org,
                                                              long long cap_segs)
{
    __shared__ SgTile s;
    __shared__ uint4 stage[kTrBlock + 1];                          // the tile's kept codes, on the 16-byte grid of their address
    const long long nseg = state[kTrN], nkept = state[kTrTotal];
    // block-uniform: the call fails (a bad table, or the segments or the bases do not fit), nothing is stored
    if (state[kSgMask] != 0 || nseg > cap_segs || nkept > cap_bases) return;
    const int t = threadIdx.x;
    const long long tile = blockIdx.x;
    const TileLane L = sg_load_tile(codes, n, lead, tile, off, nrec, s);
    const long long tile0 = tile * kTrTile - lead;
    if (tile == 0 && t == 0) seg_off[nseg] = nkept;
    // the tile's kept codes are one run of d_bases, from kept[tile]
    tile_compact(L, s.wave_total, s.text, stage, (long long)kept[tile], (long long)starts[tile], nseg, bases,
                 [&](long long sg, int k, long long at) {
                     const long long i = tile0 + 16 * t + k;
                     long long r = 0, origin = i;
                     if (off) {
                         r = sg_record_of(off, nrec, s.range[0], s.range[1], i);
                         origin = i - off[r];
                     }
                     seg_off[sg] = at;
                     seg_rec[sg] = (int32_t)r;
                     seg_org[sg] = origin;
                 },
                 [](uint8_t b) { return b; });
}

struct SegArea {
    long long *state;
    unsigned long long *kept, *starts;   // per tile: SG1, scanned in place
    TileInfo *info;
};

inline int64_t seg_layout(uint8_t *p, int64_t n_given, SegArea *a)
{
    const int64_t ntiles = tr_tiles(n_given, 15);
    Carver c{p};
    c.take(a->state, 8 * kTrStateWords);
    c.take(a->kept, 8 * (ntiles + 1));
    c.take(a->starts, 8 * (ntiles + 1));
    c.take(a->info, (int64_t)sizeof(TileInfo) * (ntiles + 1));
    return c.at;
}

// genie_segment_coords, the positions form: the segment by ctg_find, then two gathers
__global__ void __launch_bounds__(256) sg_coords_pos_kernel(DevIndex ix, CtgTab g, const int32_t *__restrict__ seg_rec,
                                                            const long long *__restrict__ seg_org, const int32_t *__restrict__ pos,
                                                            int stride, long long count, longlong2 *__restrict__ out)
{
    extern __shared__ int ctg_lds[];
    ctg_stage(g, ix.n, ctg_lds);
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int p = pos[i * stride];
    longlong2 o = make_longlong2(-1ll, -1ll);
    if (p >= 1 && p <= ix.n) {
        const CtgHit h = ctg_find(g, ctg_lds, ix.n, p - 1);
        if (h.room > 0 && p > h.start) o = make_longlong2((long long)seg_rec[h.c], seg_org[h.c] + (p - h.start));
    }
    out[i] = o;
}

// ... the hits form: (segment, 1-based offset inside it), a gather
__global__ void __launch_bounds__(256) sg_coords_hits_kernel(const long long *__restrict__ seg_off, long long nsegs,
                                                             const int32_t *__restrict__ seg_rec, const long long *__restrict__ seg_org,
                                                             const int32_t *__restrict__ in, int stride, long long count,
                                                             longlong2 *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const long long sg = in[i * stride], o = in[i * stride + 1];
    longlong2 res = make_longlong2(-1ll, -1ll);
    if (sg >= 0 && sg < nsegs && o >= 1 && o <= seg_off[sg + 1] - seg_off[sg]) res = make_longlong2((long long)seg_rec[sg], seg_org[sg] + o);
    out[i] = res;
}

}  // namespace

int64_t reference_segments_tmp_bytes(int64_t n_given, int64_t n_records)
{
    (void)n_records;                                                 // nothing is per record
    SegArea a;
    return seg_layout(nullptr, n_given, &a);
}

int launch_reference_segments(const uint8_t *d_codes, int64_t n_given, const int64_t *d_record_offsets, int64_t n_records,
                              uint8_t *d_bases, int64_t cap_bases, int64_t *d_seg_offsets, int32_t *d_seg_record, int64_t *d_seg_origin,
                              int64_t cap_segs, int64_t *out4, void *d_tmp, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int lead = (int)(reinterpret_cast<uintptr_t>(d_codes) & 15);
    const long long tiles = tr_tiles(n_given, lead);
    const long long ntiles = tiles > 0 ? tiles : 1;                  // an empty reference still writes d_seg_offsets[0]
    SegArea a;
    seg_layout(static_cast<uint8_t *>(d_tmp), n_given, &a);
    const long long *off = reinterpret_cast<const long long *>(d_record_offsets);
    dim3 tgrid;
    if (int rc = grid_for(ntiles, kTrBlock, &tgrid)) return rc;
    HIP_TRY(hipMemsetAsync(a.state, 0, 8 * kTrStateWords, s));
    if (off) {
        const long long want = (n_records + 1 + 255) / 256;
        LAUNCH(ctg_validate_kernel, dim3((unsigned)std::min(want, 2048ll)), dim3(256), 0, s, off, (long long)n_records, (long long)n_given,
               reinterpret_cast<unsigned int *>(a.state + kSgMask));
    }
    LAUNCH(sg_count_kernel, tgrid, dim3(kTrBlock), 0, s, d_codes, (long long)n_given, lead, off, (long long)n_records, a.state, a.kept,
           a.starts, a.info);
    LAUNCH(fa_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, a.kept, a.starts, a.info, ntiles, (long long)n_given, lead, 0, a.state);
    if (d_bases)
        LAUNCH(sg_compact_kernel, tgrid, dim3(kTrBlock), 0, s, d_codes, (long long)n_given, lead, off, (long long)n_records, a.state, a.kept,
               a.starts, d_bases, (long long)cap_bases, reinterpret_cast<long long *>(d_seg_offsets), d_seg_record,
               reinterpret_cast<long long *>(d_seg_origin), (long long)cap_segs);
    long long st[kTrStateWords];
    if (int rc = tr_read_state(a.state, s, st)) return rc;
    out4[0] = st[kTrN];
    out4[1] = st[kTrTotal];
    out4[2] = st[kTrLongest];
    out4[3] = st[kSgMask];
    if (st[kSgMask] != 0) return GENIE_E_INVALID;
    if (d_bases && (st[kTrN] > cap_segs || st[kTrTotal] > cap_bases)) return GENIE_E_CAPACITY;
    return GENIE_OK;
}

int launch_segment_coords(const genie_index *ix, const int64_t *d_seg_offsets, const int32_t *d_seg_record, const int64_t *d_seg_origin,
                          int64_t n_segs, int32_t form, const int32_t *d_in, int32_t stride, int64_t count, int64_t *d_out, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (count == 0) return GENIE_OK;
    const long long *org = reinterpret_cast<const long long *>(d_seg_origin);
    longlong2 *out = reinterpret_cast<longlong2 *>(d_out);
    if (form == GENIE_SEG_POSITIONS) {
        const CtgTab g = ctg_tab(d_seg_offsets, n_segs);
        LAUNCH_BLOCKS(sg_coords_pos_kernel, (count + 255) / 256, 256, ctg_lds_bytes(g), s, ix->dev, g, d_seg_record, org, d_in, (int)stride,
                      (long long)count, out);
    } else {
        LAUNCH_BLOCKS(sg_coords_hits_kernel, (count + 255) / 256, 256, 0, s, reinterpret_cast<const long long *>(d_seg_offsets),
                      (long long)n_segs, d_seg_record, org, d_in, (int)stride, (long long)count, out);
    }
    return GENIE_OK;
}

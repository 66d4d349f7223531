// short_read_kernel.inc -- traversal (K_B) and interval (K_C) kernels of the read pipeline.  Included by
// kernels.hip inside namespace genie::{anonymous}; K_A (match statistics) lives in match_table_kernel.inc.
// NARROW form (reads of at most 255 bases -- every BASELINE.json configuration): fwd[] as bytes, K_B stages
// them in LDS, one lane per read.  WIDE form (256 .. 8192 bases): fwd[] as uint16 in global memory, K_B with 8 or
// 16 lanes per read.
//
// Three kernels, because the parts of the path want different mappings:
//
//   K_A  match_table_kernel / match_table_long_kernel   A GROUP OF READS PER WAVE (long reads: one).  Matching
//        statistics fwd[a] = end of the longest prefix of read[a:] that occurs in the reference, from one
//        32-byte match-table entry per looked-up position (match_table_kernel.inc).  Writes fwd[] and the packed
//        read.
//
//   K_B  traverse_kernel<MODE>          ONE LANE PER READ.  The reference's greedy traversal is serial
//        and branchy; run wave-per-read it executes on the CU's single scalar issue port (measured:
//        ~5k scalar instructions per read).  Run lane-per-read it is ordinary SIMT code: a block stages
//        the fwd[] rows of 256 reads in LDS (odd dword stride, conflict-free) and every wave
//        instruction advances 64 reads.  It touches no index data and emits (start, end) byte pairs
//        into a compact per-read list in the workspace.
//        traverse_long_kernel<MODE, G, V>  G LANES PER READ (long reads): every step scans the window of
//        positions that still cover the current one G x V at a time -- 16 x 1 straight from global memory (small
//        batches), 2 x 8 from LDS windows of the row (batches of 32 768 reads or more).
//
//   K_C  interval_rows_kernel / interval_kernel   ONE LANE PER EMITTED SMEM.  Fills in the
//        SA interval [lo, hi] of every emitted substring: from ONE match-table entry where that decides
//        (patterns of P2 .. P2 + 16 bases; longer ones that single out one key; the longest occurring prefix
//        of an absent P2-mer; interval_from_entry), else the general bounded search over suffix-array rows, 64 at a
//        time from a per-wave list (one step for both kernels: resolve_row, WaveList); packed read from K_A's output.
//        Persistent 512-thread blocks.  Short reads in CSR
//        form: interval_rows_kernel, the rows of a tile of 256 reads densely over the lanes, the tile's slots staged in
//        LDS; long reads and the slot form: interval_kernel, 16 lanes per read.

template <bool WIDE>
struct ReadTraits {
    typedef uint8_t fwd_t;                              // fwd[] element
    static constexpr int kj_bits = 16, kj_shift = 8;   // emitted (start | end << shift) entry
};
template <>
struct ReadTraits<true> {
    typedef uint16_t fwd_t;
    static constexpr int kj_bits = 32, kj_shift = 16;
};

// ------------------------------------------------------------------ K_B
// The traversal in terms of RUNS of fwd[] (fwd[] is non-decreasing; a run start is a position whose value differs
// from the one before it; position 0 is one).  A step at `i` = SMEM.get_SMEM_at_index (SMEM.py:469-484) =
// forward_extension from i, then backward_extension (SMEM.py:389-423) over every right end i+1 .. f = fwd[i]:
//   A = (k1, f), k1 = the first position whose match reaches f = the start of the run that holds i;
//   B = the longest match fwd[k] - k among the positions k < k1 whose match still covers i, the first on ties
//       (ascending keys, strict `>` at :413); B wins a tie with A (:418-421).
// fwd[k] - k falls inside a run, so only run starts compete.  The previous step's SMEM (k', i) has fwd[k'] = i
// exactly: k' starts the run of value i, every later run has a larger value, i.e. covers i.  So the candidates of the
// step are exactly THE RUN STARTS IN (k', i], A being the last of them, and the step is
//     the first maximum of fwd[b] - b over the run starts b in (k', i]   (none, or length 0: read[i] occurs nowhere)
// -- no search at all.  Inside a run fwd[b] - b falls, so the maximum over ALL positions from the first run start behind k'
// up to i is the same one: the kernel finds that run start (the first position behind k' whose value is not i) and takes
// the maximum four positions per instruction -- a dword of the row minus the positions' own bytes is four lengths, each
// becomes a 16-bit key  length << 8 | 255 - position  (v_perm_b32), two v_pk_max_u16 keep the best (the smaller position on ties).
// (Per 10^6 x 150-base reads: 147 us walking the run starts one at a time from a bit mask, 94 us this way.)

typedef unsigned short kb_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t kb_pk_max(uint32_t a, uint32_t b)        // v_pk_max_u16
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(kb_us2, a), __builtin_bit_cast(kb_us2, b)));
}

constexpr int kPairHeadWords = 4;    // 8-byte words of a read's (count, pairs) row kept beside its packed-read records

// CSR offsets without a scan pass over the counts: the traversal kernels leave, per read, the sum of the counts of the
// reads BEFORE it in its block, and per block the block's sum; one small kernel scans the block sums
// (`scan_block_sums_kernel`), and the interval kernel adds the two -- it writes offsets[] itself.
// Every thread of the block calls this (v = 0 where there is no read); returns the exclusive prefix of v.
__device__ __forceinline__ int block_exclusive_scan(int v, int &total)
{
    __shared__ int wave_total[16];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int t = __shfl_up(inc, off, kWave);
        if (lane >= off) inc += t;
    }
    if (lane == kWave - 1) wave_total[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) {
        const int t = wave_total[w];
        before += w < wave ? t : 0;
        all += t;
    }
    total = all;
    return before + inc - v;
}

template <int MODE>
__global__ void __launch_bounds__(256) traverse_kernel(DevIndex ix, const int32_t *__restrict__ lens, long long N,
                                                        int fixed_len, int min_len, const void *__restrict__ fwd_in,
                                                        int fwd_stride, int fwd_lds,
                                                        int32_t *__restrict__ counts, void *__restrict__ kj_out, int kj_stride,
                                                        uint8_t *__restrict__ head_out, int head_stride, int cap,
                                                        int32_t *__restrict__ status, unsigned long long *__restrict__ block_sums,
                                                        uint8_t *__restrict__ counts8, uint8_t *__restrict__ status8)
{
    extern __shared__ __align__(16) uint8_t smem[];
    typedef ReadTraits<false>::fwd_t fwd_t;
    constexpr int kBits = ReadTraits<false>::kj_bits, kShift = ReadTraits<false>::kj_shift, kPer = 64 / kBits;
    const long long r0 = (long long)blockIdx.x * blockDim.x;
    {
        // stage this block's fwd[] rows: global rows are fwd_stride bytes (a multiple of 16), LDS rows fwd_lds bytes
        // -- an odd number of dwords, so lanes reading the same offset of their own rows hit distinct banks
        // 16 bytes per load, eight loads in flight per lane (one dword at a time the block spent half its life here)
        const int rows = (int)(N - r0 < (long long)blockDim.x ? N - r0 : (long long)blockDim.x);
        const uint4 *src = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(fwd_in) + r0 * (long long)fwd_stride);
        uint32_t *dst = reinterpret_cast<uint32_t *>(smem);
        const int ldw = fwd_lds >> 2, upr = fwd_stride >> 4;                       // LDS dwords / global 16-byte units per row
        const uint32_t recip = (uint32_t)((0x100000000ull + (uint64_t)upr - 1) / (uint64_t)upr);
        const int units = rows * upr;
        constexpr int kInFlight = 8;
        for (int e0 = threadIdx.x; e0 < units; e0 += kInFlight * blockDim.x) {
            uint4 v[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; u++) {
                const int e = e0 + u * blockDim.x;
                v[u] = e < units ? src[e] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < kInFlight; u++) {
                const int e = e0 + u * blockDim.x;
                if (e < units) {
                    const int row = upr > 1 ? (int)__umulhi((uint32_t)e, recip) : e;
                    const int col = 4 * (e - row * upr);
                    uint32_t *d = dst + row * ldw + col;
                    d[0] = v[u].x;                                                 // col < ldw: ldw >= 4 * upr - 3
                    if (col + 1 < ldw) d[1] = v[u].y;
                    if (col + 2 < ldw) d[2] = v[u].z;
                    if (col + 3 < ldw) d[3] = v[u].w;
                }
            }
        }
        __syncthreads();
    }
    const long long r = r0 + threadIdx.x;
    const bool valid = r < N;
    int cnt = 0;
    if (valid) {
        int st = status[r];
        const int L = lens ? lens[r] : fixed_len;
        const fwd_t *fw = reinterpret_cast<const fwd_t *>(smem + threadIdx.x * fwd_lds);       // this lane's row in LDS
        // emitted SMEMs as (start | end << 8) entries of 16 bits, packed into
        // 8-byte stores (2-byte scattered stores were amplified ~9x on their way to HBM).  Entry 0 of the row is
        // the COUNT, so that K_C learns it with the same load as the first pairs (one step less in its chain of
        // dependent loads); the row's first word is therefore written last.  The first kPairHeadWords words of the row
        // (count + 15 pairs of a short read) live in the read's slot of the packed-read records (`head_out`), the line
        // K_C fetches its window from; later words in the kj row proper.
        unsigned long long *out64 = reinterpret_cast<unsigned long long *>(reinterpret_cast<uint8_t *>(kj_out) +
                                                                           r * (long long)kj_stride * (kBits / 8));
        unsigned long long *head64 = reinterpret_cast<unsigned long long *>(head_out + r * (long long)head_stride);
        unsigned long long acc = 0, acc0 = 0;

#define EMIT(kk, jj)                                                          \
        do {                                                                      \
            const int s_ = cnt + 1;                                               \
            const unsigned long long v_ = (unsigned long long)(uint32_t)((kk) | ((jj) << kShift)) << (kBits * (s_ & (kPer - 1))); \
            if (s_ < kPer) acc0 |= v_;                                            \
            else {                                                                \
                acc |= v_;                                                        \
                if ((s_ & (kPer - 1)) == kPer - 1) { (s_ / kPer < kPairHeadWords ? head64 : out64)[s_ / kPer] = acc; acc = 0; } \
            }                                                                     \
            cnt++;                                                                \
        } while (0)

        if (st == GENIE_READ_OK && L > 0) {
            // SMEM.get_SMEMS (SMEM.py:456-467): i = 0; SMEM at i (get_SMEM_at_index :469-484); i = its end.
            // SMEM.get_smems_lut / get_smems_rmi (SMEM.py:20-192 / 206-384) produce the SAME sequence of SMEMs: their
            // K-frame state machine only decides which seed look-ups to spend; every candidate it offers is a match that
            // covers the current position, the longest such match is always among the offers and later (smaller-end)
            // offers win ties -- which is get_SMEM_at_index's answer (proof sketch + 26 M-read search: DESIGN.md section 4).
            // So all three modes run this loop; LUT / RMI differ in what they reject (reads shorter than K) and in
            // ignoring min_len (the reference's get_smems_* have no such parameter).
            int i = 0, kprev = -1;
            const uint32_t *fw32 = reinterpret_cast<const uint32_t *>(fw);
            while (i < L) {
                // s0 = the first position behind the previous SMEM's start k' whose match reaches beyond i: fwd[] is non-decreasing
                // and fwd[k'] = i, so the positions before it are the rest of k''s run, value i exactly (none up to i: read[i]
                // occurs nowhere).  Found four positions per load; every position is passed once per read.
                const int p0 = kprev + 1;
                const uint32_t i4 = (uint32_t)i * 0x01010101u;
                int sd = p0 >> 2;
                uint32_t x = (fw32[sd] ^ i4) & (~0u << (8 * (p0 & 3)));
                while (x == 0 && sd < (i >> 2)) x = fw32[++sd] ^ i4;
                const int s0 = 4 * sd + ((__ffs((int)x) - 1) >> 3);
                if (x == 0 || s0 > i) { st = GENIE_READ_ABSENT_BASE; break; }
                // the first maximum of fwd[b] - b over ALL positions b in [s0, i] (inside a run the length falls, so it is a run
                // start), four positions per step: a dword of the row minus the positions' own bytes = four lengths; every
                // position becomes a 16-bit key  length << 8 | 255 - position  (v_perm_b32), two packed maxima keep the best
                // (the first and the last dword masked to [s0, i]; the ones between need no mask)
                const uint32_t *pd = fw32 + (s0 >> 2);
                int more = (i >> 2) - (s0 >> 2);                                // dwords behind the first
                uint32_t pos = (uint32_t)(s0 >> 2) * 0x04040404u + 0x03020100u;
                uint32_t vb = ~0u << (8 * (s0 & 3));                            // positions before s0 do not compete
                const uint32_t vl = ~0u >> (8 * (3 - (i & 3)));                 // nor those behind i
                if (more == 0) vb &= vl;
                uint32_t len4 = (*pd - pos) & vb, pin4 = ~pos & vb;             // (fwd[b] >= b: no borrow between the bytes)
                uint32_t top0 = __builtin_amdgcn_perm(len4, pin4, 0x05010400u), top1 = __builtin_amdgcn_perm(len4, pin4, 0x07030602u);
                if (more > 0) {
                    while (--more > 0) {
                        pos += 0x04040404u;
                        len4 = *++pd - pos;
                        pin4 = ~pos;
                        top0 = kb_pk_max(top0, __builtin_amdgcn_perm(len4, pin4, 0x05010400u));
                        top1 = kb_pk_max(top1, __builtin_amdgcn_perm(len4, pin4, 0x07030602u));
                    }
                    pos += 0x04040404u;
                    len4 = (*++pd - pos) & vl;
                    pin4 = ~pos & vl;
                    top0 = kb_pk_max(top0, __builtin_amdgcn_perm(len4, pin4, 0x05010400u));
                    top1 = kb_pk_max(top1, __builtin_amdgcn_perm(len4, pin4, 0x07030602u));
                }
                const uint32_t mx = kb_pk_max(top0, top1);
                const uint32_t key = max(mx & 0xFFFFu, mx >> 16);
                const int best = (int)(key >> 8), bk = 255 - (int)(key & 255u);
                if (best == 0) { st = GENIE_READ_ABSENT_BASE; break; }
                if (MODE != GENIE_MODE_BWA || best >= min_len) EMIT(bk, bk + best);
                i = bk + best;
                kprev = bk;
            }
            if (st != GENIE_READ_OK) cnt = 0;
            else {
                if (cnt + 1 >= kPer && ((cnt + 1) & (kPer - 1))) ((cnt + 1) / kPer < kPairHeadWords ? head64 : out64)[(cnt + 1) / kPer] = acc;
                if (cnt > cap) st = GENIE_READ_OVERFLOW;
            }
        }
#undef EMIT
        head64[0] = cnt ? acc0 | (unsigned long long)(uint32_t)cnt : 0ull;
        status[r] = st;
        if (counts8) {                                    // compact output (genie_find_smems_packed): a byte each, 64 reads per store
            counts8[r] = (uint8_t)cnt;
            status8[r] = (uint8_t)st;
        }
    }
    // counts[]: the count (slot form), or the sum of the counts before this read in its block (CSR form)
    if (block_sums) {
        int total;
        const int before = block_exclusive_scan(cnt, total);
        if (valid) counts[r] = before;
        if (threadIdx.x == 0) block_sums[blockIdx.x] = (unsigned long long)total;
    } else if (valid) {
        counts[r] = cnt;
    }
}

// ------------------------------------------------------------------ K_B, long reads
// Reads of 256 .. 8192 bases are few and long: one lane per read leaves most of the chip idle and every step waits on
// a chain of dependent global loads.  Here G = 8 or 16 LANES work on one read.  The step is the one of the short-read
// kernel (above): the candidates are the positions in (k', i], k' the start of the previous SMEM, whose match covers
// i; the winner is the first maximum of fwd[k] - k.  (All positions take part here, not only run starts: inside a run
// the length falls, so the run start wins anyway; the positions that continue k's own run have fwd = i and do not
// cover i.)  A step loads fwd[i], fwd[i-1], ... G at a time (one 16- or 32-byte segment) down to the first position
// that no longer covers i (they are contiguous: fwd[] is non-decreasing) and keeps the
// maximum of (length << 16 | 0xFFFF - position) with a G-lane DPP reduction: the longest, the smallest position on
// ties -- SMEM.backward_extension's order (SMEM.py:413, 418-421).  Emitted pairs collect one per lane and leave as
// 4 G-byte stores.
// Every DPP source lane below lies inside the G-lane group, so `old` = 0 / bound_ctrl never show: they let the
// compiler fold the move into v_max_u32_dpp.
template <int G>
__device__ __forceinline__ uint32_t group_max(uint32_t v)
{
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true));       // quad_perm [1,0,3,2]
    if (G >= 4) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true));       // quad_perm [2,3,0,1]
    if (G >= 8) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true));      // row_half_mirror
    if (G == 16) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true));      // row_mirror
    return v;
}

// V = 8 (many reads: G = 2 or 4 lanes per read): a lane takes an aligned chunk of EIGHT positions per pass (one 16-byte load)
// instead of one position -- with eight lanes per read a wave advanced only eight reads per instruction, and the kernel took
// 0.40 ms for 75 000 x 2000 bases against 0.11 ms for the same bases as 150-base reads.
constexpr int kLongWin = 128;                             // positions per LDS window
constexpr int kLongRowBytes = 2 * kLongWin + 16;          // per read; the pad spreads the reads' rows over the banks
template <int MODE, int G, int V = 1>
__global__ void __launch_bounds__(256) traverse_long_kernel(const int32_t *__restrict__ lens, long long N, int fixed_len, int min_len,
                                                             const uint8_t *__restrict__ fwd_in, int fwd_stride,
                                                             int32_t *__restrict__ counts, uint32_t *__restrict__ kj_out,
                                                             int kj_stride, int cap, int32_t *__restrict__ status,
                                                             unsigned long long *__restrict__ block_sums)
{
    static_assert((V == 1 && (G == 8 || G == 16)) || (V == 8 && (G == 2 || G == 4)), "lanes per read / positions per lane");
    // V == 8: the row is worked through in WINDOWS of kLongWin positions staged in LDS (the rows come from HBM -- K_A's
    // non-temporal stores -- and a step's loads depend on the step before: straight from global memory every step waited
    // ~1 us for its line).  A window is loaded whole, all its loads in flight together, when a step's range leaves it.
    extern __shared__ __align__(16) uint8_t smem[];
    uint8_t *wrow = smem + (threadIdx.x / G) * kLongRowBytes;
    const int row_chunks = fwd_stride >> 4;               // 16-byte chunks (8 positions) per row
    int wb = -(1 << 20);                                  // first position of the window in LDS (none yet)
    constexpr int kShift = ReadTraits<true>::kj_shift;
    const int lane = threadIdx.x & (kWave - 1), sub = lane & (G - 1);
    const long long r = (long long)blockIdx.x * (blockDim.x / G) + (threadIdx.x / G);
    const bool valid = r < N;
    int st = valid ? status[r] : GENIE_READ_OK;
    const int L = valid ? (lens ? lens[r] : fixed_len) : 0;
    const uint16_t *fw = reinterpret_cast<const uint16_t *>(fwd_in + (valid ? r : 0) * (long long)fwd_stride);
    uint32_t *row = kj_out + (valid ? r : 0) * (long long)kj_stride;          // entry 0 = the count, then the pairs
    int i = 0, cnt = 0;
    uint32_t mine = 0;                                    // entry (cnt + 1) & ~(G - 1) | sub of the row, until it is stored
    bool go = valid && st == GENIE_READ_OK && L > 0;
    int kprev = -1;                                       // start of the previous SMEM
    // every loop below is wave-uniform (conditions are __any), so the DPP operations run with all lanes enabled
    while (__any(go)) {
        uint32_t best = 0;                                // (length << 16 | 0xFFFF - start) of the winner so far
        int top = i;
        bool more = go;
        if (V == 8) {
            // Positions at or below k' need no test of their own: fwd[k'] = i exactly and fwd[] is non-decreasing, so "the match
            // reaches beyond i" already excludes them; positions behind i are cut out of the first pass's top chunk.  A
            // position's key (length << 16 | 0xFFFF - position) is (fwd << 16) + a constant of the position.
            int ctop = i >> 3;                            // the chunk that holds i; lane `sub` of a pass takes chunk ctop - sub
            const uint32_t reach = ((uint32_t)i << 16) | 0xFFFFu;                       // (v << 16) > reach  <=>  v > i
            bool first = true;
            // the window must hold the chunk of k' + 1 up to the chunk of i (a range longer than a window: global loads)
            const int need_lo = (kprev + 1) & ~7;
            const bool fits = go && i - need_lo < kLongWin;
            const bool reload = fits && !(need_lo >= wb && i < wb + kLongWin);
            if (__any(reload)) {
                if (reload) {
                    wb = need_lo;
                    uint4 t[kLongWin / 8 / G];
#pragma unroll
                    for (int u = 0; u < kLongWin / 8 / G; u++) {
                        const int c = (wb >> 3) + sub + G * u;
                        t[u] = c < row_chunks ? *reinterpret_cast<const uint4 *>(fw + 8 * c) : make_uint4(0, 0, 0, 0);
                    }
#pragma unroll
                    for (int u = 0; u < kLongWin / 8 / G; u++) *reinterpret_cast<uint4 *>(wrow + 16 * (sub + G * u)) = t[u];
                }
                wave_lds_fence();
            }
            while (__any(more)) {
                const int c = ctop - sub;
                const bool inb = more && c >= 0;
                uint4 q = make_uint4(0, 0, 0, 0);
                if (inb) {
                    if (fits && 8 * c >= wb) q = *reinterpret_cast<const uint4 *>(wrow + 2 * (8 * c - wb));   // (8 c <= i < wb + kLongWin)
                    else q = *reinterpret_cast<const uint4 *>(fw + 8 * c);              // rows are 16-byte aligned
                }
                uint32_t qd[4] = {q.x, q.y, q.z, q.w};
                if (first) {                                                             // wave-uniform
                    const int jmax = (sub == 0) ? (i & 7) : 7;                           // positions behind i do not compete
#pragma unroll
                    for (int d = 0; d < 4; d++) qd[d] &= jmax >= 2 * d + 1 ? 0xFFFFFFFFu : (jmax >= 2 * d ? 0x0000FFFFu : 0u);
                    first = false;
                }
                const uint32_t c0 = (uint32_t)(0xFFFF - 8 * c) - ((uint32_t)(8 * c) << 16);
                uint32_t kmax = 0;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const uint32_t vh = (j & 1) ? (qd[j >> 1] & 0xFFFF0000u) : (qd[j >> 1] << 16);
                    const uint32_t key = vh > reach ? vh + (c0 - (uint32_t)j * 0x10001u) : 0u;
                    kmax = max(kmax, key);
                }
                best = max(best, group_max<G>(kmax));
                const bool low = inb && (qd[0] << 16) > reach;                           // the pass's lowest position still covers i
                ctop -= G;
                more = more && ((__ballot(low) >> (lane | (G - 1))) & 1ull);
            }
        }
        while (V == 1 && __any(more)) {
            const int k = top - sub;
            const bool in = more && k > kprev;
            const int v = in ? (int)fw[k] : 0;
            const bool covers = in && v > i;              // contiguous down from i: fwd[] is non-decreasing
            const uint32_t key = covers ? ((uint32_t)(v - k) << 16) | (uint32_t)(0xFFFF - k) : 0u;
            best = max(best, group_max<G>(key));
            top -= G;
            more = more && ((__ballot(covers) >> (lane | (G - 1))) & 1ull);   // the pass's last position still covers i
        }
        if (go) {
            const int blen = (int)(best >> 16), bk = 0xFFFF - (int)(best & 0xFFFFu);
            if (blen == 0) { st = GENIE_READ_ABSENT_BASE; go = false; }       // nothing covers i: read[i] occurs nowhere
            else {
                if (MODE != GENIE_MODE_BWA || blen >= min_len) {
                    const int s_ = cnt + 1;
                    if (sub == (s_ & (G - 1))) mine = (uint32_t)(bk | ((bk + blen) << kShift));
                    if ((s_ & (G - 1)) == G - 1) {
                        const int idx = (s_ & ~(G - 1)) + sub;
                        if (idx > 0) row[idx] = mine;
                    }
                    cnt++;
                }
                kprev = bk;
                i = bk + blen;
                go = i < L;
            }
        }
    }
    if (valid) {
        if (st != GENIE_READ_OK) cnt = 0;
        else {
            const int idx = ((cnt + 1) & ~(G - 1)) + sub;
            if (((cnt + 1) & (G - 1)) != 0 && idx >= 1 && idx <= cnt) row[idx] = mine;
            if (cnt > cap) st = GENIE_READ_OVERFLOW;
        }
        if (sub == 0) {
            row[0] = (uint32_t)cnt;
            status[r] = st;
        }
    }
    if (block_sums) {                                     // CSR form: see block_exclusive_scan
        int total;
        const int before = block_exclusive_scan(valid && sub == 0 ? cnt : 0, total);
        if (valid && sub == 0) counts[r] = before;
        if (threadIdx.x == 0) block_sums[blockIdx.x] = (unsigned long long)total;
    } else if (valid && sub == 0) {
        counts[r] = cnt;
    }
}

// ------------------------------------------------------------------ K_C
// Final rows (start, end, lo, hi), each written exactly once.  CSR = false: row t of read r goes to slots[r*cap + t]
// (t < cap); CSR = true:  to out[offsets[r] + t] (offsets = exclusive scan of the counts, rows past out_cap dropped).
//
// Patterns of P2 .. P2 + 16 bases whose match-table entry is not slow (most SMEMs) are answered on the spot from
// that ONE entry: it holds the first row of the P2-mer and the 16-base continuation of each of (up to six of) its
// suffixes in suffix-array order, so the rows that carry the pattern are those whose key agrees with it that far.
// Everything else (shorter, longer, slow entries) goes onto a per-wave list and is searched 64 at a time with the
// general interval search -- so that its (long) code runs on full waves, not on the odd lane of every wave.
// That step is resolve_row (below), the same for interval_kernel (a row per lane of a read's 16) and interval_rows_kernel
// (a row per lane); its entry half, interval_from_window, also gives lr_ms_kernel (long_reads.inc) its intervals.
constexpr int kIvWaves = 8;          // waves per block
constexpr int kIvList = 128;         // list entries per wave: fewer than 64 pending + at most 64 appended at once

// Final row: (start, end, lo, hi) as four int32 (COUT = 0), or the compact forms of genie_find_smems_packed / _packed6:
//   COUT = 1, 8 bytes: start | end << 8 | span << 16, lo;  span = hi - lo, 0xFFFF = 65535 or more;
//   COUT = 2, 6 bytes: start, end, lo in 24 bits, span in 8 bits, 0xFF = 255 or more (references below 2^24 bases);
// a row whose span does not fit also puts (row index, hi) onto the escape list.
struct RowEscapes {
    unsigned long long *count;      // [1]: escapes so far (may exceed cap: the caller compares)
    long long *list;                // [2 * cap]: row index, hi
    long long cap;
};
template <int COUT>
__device__ __forceinline__ void emit_row(void *out, long long idx, int k, int j, int lo, int hi, const RowEscapes &esc)
{
    if (COUT == 0) {
        store_nt(reinterpret_cast<int4 *>(out) + idx, make_uint4((uint32_t)k, (uint32_t)j, (uint32_t)lo, (uint32_t)hi));   // final rows: nobody here reads them again
        return;
    }
    constexpr uint32_t kTop = COUT == 1 ? 0xFFFFu : 0xFFu;
    uint32_t span = (uint32_t)(hi - lo);
    if (span >= kTop) {
        const unsigned long long slot = atomicAdd(esc.count, 1ull);
        if ((long long)slot < esc.cap) {
            esc.list[2 * slot] = idx;
            esc.list[2 * slot + 1] = hi;
        }
        span = kTop;
    }
    if (COUT == 1) {
        reinterpret_cast<uint2 *>(out)[idx] = make_uint2((uint32_t)k | (uint32_t)j << 8 | span << 16, (uint32_t)lo);
    } else {
        uint16_t *o = reinterpret_cast<uint16_t *>(out) + 3 * idx;               // rows are 2-byte aligned
        o[0] = (uint16_t)((uint32_t)k | (uint32_t)j << 8);
        o[1] = (uint16_t)lo;
        o[2] = (uint16_t)(((uint32_t)lo >> 16) | span << 8);
    }
}

// What ONE match-table entry (`ra`, and `rb` of the 32-byte form) says about the pattern of `len` bases whose window is `w`:
// true and its rows in `iv` where the entry decides, false where the general search must.
template <bool C16>
__device__ __forceinline__ bool interval_from_entry(const int4 ra, const int4 rb, uint64_t w, int len, int P2,
                                                    const __amdgpu_buffer_rsrc_t ov, bool act, int2 &iv)
{
    const uint32_t meta = (uint32_t)ra.x;
    // every pattern here is an emitted SMEM, so it OCCURS: (a) an absent P2-mer whose longest occurring
    // prefix is the pattern -> that prefix's rows, kept in the entry; (b) P2 .. P2 + 16 bases -> the keys
    // that agree that far; (c) longer, with ONE key agreeing in all 16 bases -> that row.
    bool fast = false;
    iv = make_int2(-1, -1);
    if (C16) {
        // compact entry (genie_internal.h): the same three cases with 8-base keys; an entry of more than
        // six suffixes continues in the per-row key array
        const uint32_t cnt4 = (meta >> 24) & 15u, nib = meta >> 28, lb = meta & 0xFFFFFFu;
        if (act && cnt4 == 0) {
            if (len == (int)nib) { fast = true; iv = make_int2((int)lb, ra.y); }
        } else if (act && (nib & kM16Wide) && cnt4 <= 3u && len >= P2) {          // three 16-base keys
            const uint32_t xk = (uint32_t)((w << (2 * P2)) >> 32);
            const int cl = len - P2 < 16 ? len - P2 : 16;
            const uint32_t km = cl == 0 ? 0u : ~0u << (32 - 2 * cl);
            const uint32_t bits = (((((uint32_t)ra.y ^ xk) & km) == 0 ? 1u : 0u) | ((((uint32_t)ra.z ^ xk) & km) == 0 ? 2u : 0u) |
                                   ((((uint32_t)ra.w ^ xk) & km) == 0 ? 4u : 0u)) & ((1u << cnt4) - 1u);
            fast = len <= P2 + 16 || __popc(bits) == 1;
            if (bits) {
                const int first = (int)lb + __ffs((int)bits) - 1;
                iv = make_int2(first, first + __popc(bits) - 1);
            }
        } else if (act && (cnt4 == kM16More || !(nib & kM16General)) && len >= P2) {
            const uint32_t total = cnt4 == kM16More ? 7u + nib : cnt4;
            const uint32_t xk16 = (uint32_t)((w << (2 * P2)) >> 48);
            const int cl = len - P2 < 8 ? len - P2 : 8;
            const uint32_t km16 = cl == 0 ? 0u : (0xFFFFu << (16 - 2 * cl)) & 0xFFFFu;
            const uint32_t k16[6] = {(uint32_t)ra.y & 0xFFFFu, (uint32_t)ra.y >> 16, (uint32_t)ra.z & 0xFFFFu,
                                     (uint32_t)ra.z >> 16, (uint32_t)ra.w & 0xFFFFu, (uint32_t)ra.w >> 16};
            const uint32_t ninl = cnt4 == kM16More ? (uint32_t)kM16Keys - 1u : cnt4;
            uint32_t bits = 0, xm = 0xFFFFu;
#pragma unroll
            for (int i = 0; i < kM16Keys; i++) bits |= (((k16[i] ^ xk16) & km16) == 0 && (uint32_t)i < ninl) ? 1u << i : 0u;
            if (cnt4 == kM16More) mt_ov_scan(ov, k16[5], (int)total - (kM16Keys - 1), xk16, km16, xm, bits);
            fast = len <= P2 + 8 || __popc(bits) == 1;
            if (bits) {                                  // adjacent rows: the keys ascend
                const int first = (int)lb + __ffs((int)bits) - 1;
                iv = make_int2(first, first + __popc(bits) - 1);
            }
        }
    } else if (act && !(meta & kMatchSlow)) {
        const uint32_t rows = meta >> 24;
        if (rows == 0) {
            if (len == (int)(meta & 0xFFu)) { fast = true; iv = make_int2(ra.y, ra.z); }
        } else if (len >= P2) {
            const uint32_t xk = (uint32_t)((w << (2 * P2)) >> 32);
            const int cl = len - P2 < 16 ? len - P2 : 16;
            const uint32_t km = cl == 0 ? 0u : ~0u << (32 - 2 * cl);
            uint32_t bits = ((((uint32_t)ra.z ^ xk) & km) == 0 ? 1u : 0u) | ((((uint32_t)ra.w ^ xk) & km) == 0 ? 2u : 0u) |
                            ((((uint32_t)rb.x ^ xk) & km) == 0 ? 4u : 0u) | ((((uint32_t)rb.y ^ xk) & km) == 0 ? 8u : 0u) |
                            ((((uint32_t)rb.z ^ xk) & km) == 0 ? 16u : 0u) | ((((uint32_t)rb.w ^ xk) & km) == 0 ? 32u : 0u);
            bits &= (1u << rows) - 1u;                   // rows <= kMatchKeys: the entry is not slow
            fast = len <= P2 + 16 || __popc(bits) == 1;
            if (bits) {                                  // adjacent rows: the keys ascend
                const int first = (int)ra.y + __ffs((int)bits) - 1;
                iv = make_int2(first, first + __popc(bits) - 1);
            }
        }
    }
    return fast;
}

// The overflow blocks of the compact table as a buffer resource (mt_ov_scan's loads are bounds-checked by it).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mt_ov_rsrc(const DevIndex &ix)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<MatchOv16 *>(ix.ov), 0, ix.ov_entries * (int)sizeof(MatchOv16), 0x00020000);
}

// The match-table entry of the P2-mer `code`: 16 bytes (`ra`) of the compact form, 32 (`ra`, `rb`) of the full one; zeros
// for a lane that is not `act`.
template <bool C16>
__device__ __forceinline__ void mt_load_entry(const DevIndex &ix, uint32_t code, bool act, int4 &ra, int4 &rb)
{
    const int4 *en = C16 ? reinterpret_cast<const int4 *>(reinterpret_cast<const MatchRec16 *>(ix.mtab) + code)
                         : reinterpret_cast<const int4 *>(ix.mtab + code);
    ra = make_int4(0, 0, 0, 0);
    rb = make_int4(0, 0, 0, 0);
    if (act) { ra = en[0]; if (!C16) rb = en[1]; }
}

// The entry half of a row: the pattern's window -> its P2-mer's entry -> interval_from_entry (also lr_ms_kernel's).
template <bool C16>
__device__ __forceinline__ bool interval_from_window(const DevIndex &ix, uint64_t w, int len, bool act, int2 &iv)
{
    int4 ra, rb;
    mt_load_entry<C16>(ix, (uint32_t)(w >> (64 - 2 * ix.P2)), act, ra, rb);
    return interval_from_entry<C16>(ra, rb, w, len, ix.P2, mt_ov_rsrc(ix), act, iv);
}

// A wave's list of the rows that wait for the general search, {row index lo, hi, read, start | end << 16} in LDS, with
// what the search needs: the packed reads as K_A left them (QIn: QRecs / QPlain, kernels.hip) and where the rows go.
template <int COUT, class QIn>
struct WaveList {
    const DevIndex &ix;
    const RefRec *qp_in;
    int qp_stride;
    void *out;
    RowEscapes esc;
    int4 *list;                      // kIvList entries
    int nlist;

    // the general search of list[o .. o + n), n <= 64
    __device__ __forceinline__ void search(int o, int n) const
    {
        const int lane = threadIdx.x & (kWave - 1);
        if (lane < n) {
            const int4 en = list[o + lane];
            const int k = en.w & 0xFFFF, j = (int)((uint32_t)en.w >> 16);
            const QIn qp{reinterpret_cast<decltype(QIn::p)>(qp_in + (long long)en.z * qp_stride)};
            const int2 iv = sa_interval(ix, ix.dir, qp, k, j - k);
            emit_row<COUT>(out, ((long long)en.y << 32) | (uint32_t)en.x, k, j, iv.x, iv.y, esc);
        }
    }
    // The lanes with `general` append their row, in lane order; 64 or more pending: the last 64 are searched.  Called by the
    // whole wave.
    __device__ __forceinline__ void append(bool general, long long row, int read, int k, int j)
    {
        const int lane = threadIdx.x & (kWave - 1);
        const unsigned long long gb = __ballot(general);
        if (gb) {
            if (general)
                list[nlist + __popcll(gb & ((1ull << lane) - 1ull))] = make_int4((int)(uint32_t)row, (int)(row >> 32), read, k | (j << 16));
            nlist += __popcll(gb);
            wave_lds_fence();
            if (nlist >= 64) {
                nlist -= 64;
                search(nlist, 64);
                wave_lds_fence();
            }
        }
    }
    // what is left when the kernel ends
    __device__ __forceinline__ void drain() const
    {
        if (nlist) search(0, nlist);
    }
};

// ONE ROW: the pattern [k, j) of `read`, whose window is `w`, to row `row` -- from its table entry where that decides, else
// onto the wave's list.  Called by the whole wave (`act`: the lane has a row).
template <bool C16, int COUT, class QIn>
__device__ __forceinline__ void resolve_row(bool act, uint64_t w, int k, int j, long long row, int read, WaveList<COUT, QIn> &wl)
{
    int2 iv;
    const bool fast = interval_from_window<C16>(wl.ix, w, j - k, act, iv);
    if (fast) emit_row<COUT>(wl.out, row, k, j, iv.x, iv.y, wl.esc);
    wl.append(act && !fast, row, read, k, j);
}

// Long reads (WIDE) and the slot form, 16 LANES PER READ, a read's rows 16 lanes x 16 B contiguous; the CSR forms of short
// reads run interval_rows_kernel (below).  One read per 16-lane group and iteration (measured: 1 at 8 waves per SIMD beats 2 at 6; the kernel is bound by the
// chain of dependent loads count+pair -> window -> entry -> row, whose stages add up).
template <bool CSR, bool WIDE, bool C16>
__global__ void __launch_bounds__(kIvWaves * 64, 8) interval_kernel(DevIndex ix, long long N,
                                                                    const void *__restrict__ kj_in, int kj_stride,
                                                                    const uint8_t *__restrict__ head_in, int head_stride,
                                                                    const RefRec *__restrict__ qp_in, int qp_stride,
                                                                    void *__restrict__ out, int cap,
                                                                    long long *__restrict__ offsets, long long out_cap,
                                                                    const unsigned long long *__restrict__ block_base,
                                                                    const int32_t *__restrict__ before_in_block, int block_shift,
                                                                    int sched)
{
    static_assert(WIDE || !CSR, "short reads, CSR rows: interval_rows_kernel");
    __shared__ int4 lists[kIvWaves][kIvList];
    typedef typename std::conditional<WIDE, uint32_t, uint16_t>::type kj_t;
    typedef typename std::conditional<WIDE, QRecs, QPlain>::type QIn;      // how K_A left the packed read (kernels.hip)
    constexpr int kHeadEntries = kPairHeadWords * 8 / (int)sizeof(kj_t), kShift = ReadTraits<WIDE>::kj_shift;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const int sub = lane & 15;
    WaveList<0, QIn> wl{ix, qp_in, qp_stride, out, RowEscapes{}, lists[wave], 0};      // four-int32 rows: no escapes
    const long long step = (long long)gridDim.x * kIvWaves * 4;
    // (issue priority rotated per iteration, as in the match-statistics kernel: the CU serves its oldest waves first)
    const bool rotate = !(sched & 1);
    int it = (int)(blockIdx.x / (uint32_t)(sched >> 8));
    for (long long r0 = ((long long)blockIdx.x * kIvWaves + wave) * 4; r0 < N; r0 += step, it++) {
        if (rotate) set_wave_priority(it);
        const bool have = r0 + (lane >> 4) < N;
        const long long r = have ? r0 + (lane >> 4) : 0;
        const kj_t *head = reinterpret_cast<const kj_t *>(head_in + r * (long long)head_stride);
        // the row's entry 0 is the count
        int c = have ? (int)head[0] : 0;
        // CSR: the row offset of a read = scanned sum of the traversal blocks before its block + the counts before
        // it inside the block; written out here (offsets[N] by whoever holds the last read)
        const long long base = CSR ? (have ? (long long)block_base[r >> block_shift] + before_in_block[r] : 0) : r * (long long)cap;
        if (CSR && have && sub == 0) {
            offsets[r] = base;
            if (r == N - 1) offsets[N] = base + c;
        }
        if (!CSR) c = c < cap ? c : cap;
        for (int t0 = 0; __any(t0 < c); t0 += 16) {
            const int t = t0 + sub;
            const bool act = t < c && (!CSR || base + t < out_cap);
            const kj_t *row = t + 1 < kHeadEntries ? head : reinterpret_cast<const kj_t *>(kj_in) + r * (long long)kj_stride;
            const uint32_t e = act ? (uint32_t)row[t + 1] : 0u;
            const int k = (int)(e & ((1u << kShift) - 1)), j = (int)(e >> kShift);
            const uint64_t w = act ? QIn{reinterpret_cast<decltype(QIn::p)>(qp_in + r * (long long)qp_stride)}.win(k) : 0ull;
            resolve_row<C16>(act, w, k, j, base + t, (int)r, wl);
        }
    }
    wl.drain();
}

// ------------------------------------------------------------------ K_C, short reads, CSR rows
// ONE LANE PER ROW over staged read tiles.  The kernel above gives every read 16 lanes whatever its count, repeats the
// addressing of slot, head and offsets every four reads, and reaches its table entry through two loads that come from HBM
// (head, window).  Here a persistent block takes TILES of `tile_reads` (at most kIvTile) consecutive reads -- the host cuts
// the batch so that every block gets the same number of tiles:
//   1. it copies the tile's slots (packed read + head of the pairs row: contiguous, 16-byte aligned) into LDS, 16 bytes per
//      lane and all loads in flight together, with the tile's counts-before-the-read;
//   2. one lane per read writes offsets[] and leaves in LDS the read's first row, relative to the tile's, and its own index
//      for every 64th row of the tile that is one of its rows (chunk_read);
//   3. the tile's rows are worked through in chunks of 64 per wave: a row finds its read by bisecting the starts between
//      the reads of its chunk's first row and of the next chunk's (a handful: three steps, not eight), takes its pair and
//      its window from LDS, loads ONE table entry, and stores at tile base + row -- a wave's stores are consecutive rows.
// From the window on a row takes interval_kernel's step (resolve_row); the wave's list outlives a tile, so its search reads
// the packed read from global memory.  Rows and offsets are those of interval_kernel; the packed forms (COUT) add totals
// and escapes.
constexpr int kIvTile = 256;         // most reads per tile (tiles need not be traversal blocks)
constexpr int kIvChunks = kIvTile * 255 / kWave + 2;                               // 64-row chunks of a tile's rows, and one
constexpr int kIvRowsStaticLds = kIvWaves * kIvList * 16 + 2 * kIvTile * 4 + ((kIvChunks + 15) & ~15) + 16;   // lists, starts, chunk_read, row count

template <bool C16, int COUT>
__global__ void __launch_bounds__(kIvWaves * 64, 8) interval_rows_kernel(DevIndex ix, long long N,
                                                                         const uint16_t *__restrict__ kj_in, int kj_stride,
                                                                         const RefRec *__restrict__ qp_in, int qp_stride, int qp_recs,
                                                                         void *__restrict__ out,
                                                                         long long *__restrict__ offsets, long long out_cap,
                                                                         const unsigned long long *__restrict__ block_base,
                                                                         const int32_t *__restrict__ before_in_block, int block_shift,
                                                                         RowEscapes esc, int sched, int tile_reads)
{
    extern __shared__ __align__(16) uint8_t smem[];      // the tile's slots: kIvTile x qp_stride x 16 bytes
    __shared__ int4 lists[kIvWaves][kIvList];            // {row index lo, hi, read, start | end << 16}
    __shared__ int starts[2 * kIvTile];                  // first row of every read of the tile, relative to the tile's first;
                                                         // beyond the tile's reads: INT_MAX (a bisection may look that far)
    __shared__ uint8_t chunk_read[kIvChunks];            // the read that row 64 c of the tile belongs to
    __shared__ int tile_rows;
    constexpr int kHeadEntries = kPairHeadWords * 8 / 2;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const int slot_bytes = qp_stride * 16, head_off = qp_recs * 16;
    WaveList<COUT, QPlain> wl{ix, qp_in, qp_stride, out, esc, lists[wave], 0};
    // (issue priority rotated per tile, as in the match-statistics kernel: the CU serves its oldest waves first)
    const bool rotate = !(sched & 1);
    int it = (int)(blockIdx.x / (uint32_t)(sched >> 8));
    const long long tiles = (N + tile_reads - 1) / tile_reads;
    if ((int)threadIdx.x < kIvTile) starts[kIvTile + threadIdx.x] = 0x7FFFFFFF;      // (the barriers of the first tile order this)
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x, it++) {
        if (rotate) set_wave_priority(it);
        const long long r0 = tile * tile_reads;
        const int reads = (int)(N - r0 < (long long)tile_reads ? N - r0 : (long long)tile_reads);
        // the tile's first row (block-uniform) and, one lane per read, the read's own
        const long long tile_base = (long long)block_base[r0 >> block_shift] + before_in_block[r0];
        const bool have = (int)threadIdx.x < reads;
        const long long r = r0 + (have ? (int)threadIdx.x : 0);
        const long long base = have ? (long long)block_base[r >> block_shift] + before_in_block[r] : 0;
        {
            const uint4 *src = reinterpret_cast<const uint4 *>(qp_in + r0 * (long long)qp_stride);
            uint4 *dst = reinterpret_cast<uint4 *>(smem);
            const int units = reads * qp_stride;
            constexpr int kInFlight = 4;
            for (int e0 = threadIdx.x; e0 < units; e0 += kInFlight * kIvWaves * kWave) {
                uint4 v[kInFlight];
#pragma unroll
                for (int u = 0; u < kInFlight; u++) {
                    const int e = e0 + u * kIvWaves * kWave;
                    v[u] = e < units ? src[e] : make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < kInFlight; u++) {
                    const int e = e0 + u * kIvWaves * kWave;
                    if (e < units) dst[e] = v[u];
                }
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < kIvTile) {
            // entry 0 of the head is the count; offsets[N] (the packed forms: word 0 of the totals) by whoever holds the last read
            const int c = have ? (int)*reinterpret_cast<const uint16_t *>(smem + threadIdx.x * slot_bytes + head_off) : 0;
            if (have) {
                if (!COUT) offsets[r] = base;
                if (r == N - 1) offsets[COUT ? 0 : N] = base + c;
            }
            const int first = have ? (int)(base - tile_base) : 0x7FFFFFFF;
            starts[threadIdx.x] = first;
            // every 64th row of the tile belongs to one read with rows; the last read also answers for the first such row
            // behind the tile's rows, which bounds the last chunk
            if (have)
                for (int ch = (first + kWave - 1) >> 6; (ch << 6) < first + c; ch++) chunk_read[ch] = (uint8_t)threadIdx.x;
            if (have && (int)threadIdx.x == reads - 1) {
                tile_rows = first + c;
                chunk_read[(first + c + kWave - 1) >> 6] = (uint8_t)threadIdx.x;
            }
        }
        __syncthreads();
        const int total = tile_rows;
        for (int q0 = wave * kWave; q0 < total && tile_base + q0 < out_cap; q0 += kIvWaves * kWave) {
            const int q = q0 + lane;
            const bool act = q < total && tile_base + q < out_cap;
            // the read of row q: the last one that starts at or before it (reads without rows share their successor's start),
            // which lies between the read of the chunk's first row and that of the next chunk's: every later read starts
            // behind this chunk, so the bisection needs no upper bound
            const int lo = rfl((int)chunk_read[q0 >> 6]), span = rfl((int)chunk_read[(q0 >> 6) + 1]) - lo;
            int i = lo;
            for (int s = span > 0 ? 1 << (31 - __builtin_clz(span)) : 0; s > 0; s >>= 1) i += starts[i + s] <= q ? s : 0;
            const int t = act ? q - starts[i] : 0;
            const uint8_t *slot = smem + i * slot_bytes;
            uint32_t e = 0;
            if (act) e = t + 1 < kHeadEntries ? (uint32_t)reinterpret_cast<const uint16_t *>(slot + head_off)[t + 1]
                                              : (uint32_t)kj_in[(r0 + i) * (long long)kj_stride + t + 1];
            const int k = (int)(e & 0xFFu), j = (int)(e >> 8);
            // the window QPlain::win returns: words k / 32 and k / 32 + 1 of the slot
            const uint64_t *wp = reinterpret_cast<const uint64_t *>(slot) + (k >> 5);
            const uint64_t w = act ? funnel(wp[0], wp[1], (k & 31) * 2) : 0ull;
            resolve_row<C16>(act, w, k, j, tile_base + q, (int)(r0 + i), wl);
        }
        __syncthreads();                                  // the next tile overwrites the slots and the starts
    }
    wl.drain();
}

// match_table_kernel.inc -- K_A, the match-statistics kernel.  Included by kernels.hip inside
// namespace genie::{anonymous}, after short_read_kernel.inc.
//
// fwd[a] = end of the longest prefix of read[a:] that occurs in the reference (SURVEY.md 8a: everything the
// reference's forward_extension / `in lut` / check_sequential ask of the index follows from it).
//
// What bounds the kernel (PMC, DESIGN.md section 4): the rate of random L1->L2 requests -- one 64-byte line per
// table entry looked up, about 64 of them in flight per CU at ~220 cycles each -- and vector-instruction issue.
// So it is written to look up as few positions, and to spend as few wave instructions per read, as it can:
// every stage works on a GROUP of reads per wave, flattened over the 64 lanes.
//
//   pack     16 bases per lane -> one big-endian dword of the 2-bit stream; the stream is kept in LDS shifted
//            right by ONE bit, so that a window at any base starts at an odd bit and is two v_alignbit
//            (never a shift by 32); the 16-byte packed-read records K_B / K_C use go out from the same data.
//   lookup   the P2-mer at a position selects ONE match-table entry (MatchRec16, 16 bytes, or MatchRec, 32 bytes:
//            genie_internal.h); the longest match is  min(base + max_i lcp(continuation, key_i), bases left)  =
//            six xor, a min tree, one count-leading-zeros; a 32-byte entry mostly needs its first 16 bytes only.
//            Reads are zero padded, so the last P2-1 positions need nothing special.
//   samples  fwd[] is non-decreasing.  A lane owns four consecutive positions (a "quad"): round 1 looks up the
//            first of each quad; round 2 works inside a quad ONLY where its sample and the next quad's differ
//            (otherwise the quad shares that value): the middle position, then a neighbour only where the middle
//            does not settle it -- about 100 lookups for a 150-base read made of
//            ~10 reference segments, about 40 for one that matches end to end, 150 for a random one.
//   slow     where an entry cannot decide:
//              a key agrees in all 16 bases and more of the read is left  ->  compare with the suffix-array
//                  rows whose keys agree (inline 32-base key, then the packed reference);
//              a slow entry (more than six suffixes, or one cut short by the end of the reference)  ->
//                  bounded bisection over the P2-mer's rows (second-level table entry = bounds + first probe;
//                  RMI mode: the staged models' prediction is the next probe -- the last-mile search of
//                  RMI_LUT.get_suffix_rmi, fenced by the bucket).
//   out      fwd rows copied out 16 bytes per lane.
// No prefix directory; block-wide in LDS only the group counter and the quad table (one barrier, at the start).
//
// Two table forms (genie_internal.h), one code: C16 = true, the compact 16-byte entries (8-base keys; 16-base keys in
// entries of up to three suffixes) -- the default; C16 = false, the 32-byte entries with 16-base keys (references of 2^24
// bases or more).  On a table that does not fit the L2 the kernel's
// time follows its L2 MISSES (TCC counters, tools/experiments/README.md: 74 per read on the 1 Mb reference, and 1.27x the
// time at 1.24x the misses with a table four times larger), not its requests, so the table is halved and a lookup is one
// 16-byte load; what the short keys cannot decide (a match of more than P2 + 8 bases) is decided by the suffix-array
// rows whose keys agree, as in the 32-byte form.

// match_table_kernel comes in builds of the same code for WPS waves per SIMD (plan_find_smems picks): 6 for the compact
// table (74 VGPRs, nothing spilled, three 512-thread blocks per CU: the CU's miss queue is full with their requests, and
// the 64-register build's ten spilled registers cost 2 % at 100 kb and 7 % at 1 Mb), 4 (two blocks per CU) where the table
// exceeds an XCD's L2 -- fewer waves thrash the L2 less -- and 8 for the 32-byte form.
constexpr int kMtNsp = 3;          // quads per lane per pass
constexpr int kMtMaxG = 16;        // reads per wave iteration: chosen by the launch plan, at most this
constexpr int kMtTarget = 768;     // ... so that a group holds about this many positions (one pass of 3 x 64 quads)


__host__ __device__ inline int mt_row_dwords(int max_len, int qp_recs)
{
    const int a = ((2 * (max_len + 8) + 1) >> 5) + 3, b = 2 * qp_recs + 3;
    return a > b ? a : b;
}
__host__ __device__ inline int mt_pack_dwords(int max_len) { return (max_len + 15) / 16 + 1; }   // written per iteration
__host__ __device__ inline int mt_quads(int max_len) { return (max_len + 3) / 4; }
// per-wave scratch, every piece a multiple of 16 bytes:
//   packed reads | lengths | fwd rows | slow list | round-2 lists
__host__ __device__ inline int mt_r16(int x) { return (x + 15) & ~15; }
// per block: what round 1 and round 2's first pass need to know about quad t of a group -- the same for every group, so it is
// worked out once (entries for whole round-1 passes of 3 x 64 quads)
__host__ __device__ inline int mt_quad_table_bytes(int grp, int max_len) { return (grp * mt_quads(max_len) + 191) / 192 * 192 * 8; }
// short reads: the workspace gets the packed read as PLAIN 64-bit words, `chunks` 16-byte pieces of two (chunk j reads the
// shifted dwords 4j .. 4j+4)
__host__ __device__ inline int mt_short_row_dwords(int max_len, int chunks) { return mt_row_dwords(max_len, 2 * chunks - 1); }
__host__ __device__ inline int mt_wave_bytes(int grp, int max_len, int qp_recs, int fwd_stride)
{
    return mt_r16(grp * mt_short_row_dwords(max_len, qp_recs) * 4) + 64 + mt_r16(grp * fwd_stride) + mt_r16(grp * max_len * 2) +
           mt_r16(grp * mt_quads(max_len) * 6);          // round 2's lists: the quads to work on (2 B each), their open neighbours (2 x 2 B)
}

// The packed read in LDS: dwords of the big-endian 2-bit base stream shifted right by one bit.
struct QBits {
    const uint32_t *p;
    __device__ __forceinline__ uint64_t win(int pos) const              // 32 bases from `pos`
    {
        const uint32_t o = 2u * (uint32_t)pos + 1u;
        const uint32_t *d = p + (o >> 5);
        const uint32_t s = 32u - (o & 31u);                                // 1 .. 31
        const uint32_t d0 = d[0], d1 = d[1], d2 = d[2];
        return ((uint64_t)__builtin_amdgcn_alignbit(d0, d1, s) << 32) | __builtin_amdgcn_alignbit(d1, d2, s);
    }
};

// b0 | b1 << 8 | b2 << 16 | b3 << 24 (bases 0..3)  ->  b0 << 6 | b1 << 4 | b2 << 2 | b3 in the low byte
__device__ __forceinline__ uint32_t mt_pack4(uint32_t v) { return ((v << 6) | (v >> 4) | (v >> 14) | (v >> 24)) & 255u; }

// One table lookup, in two halves so that several can be in flight: issue (the entry's first 16 bytes; the whole
// entry in the compact form) ...
struct MtProbe {
    uint32_t xk;      // the 16 bases after the P2-mer
    int voff;         // byte offset of the entry
    mt_v4i ra;        // meta, lb, key[0..1]  /  the compact entry
};
template <bool C16>
__device__ __forceinline__ MtProbe mt_issue(const __amdgpu_buffer_rsrc_t mtab, uint32_t w1, uint32_t w2, int P2)
{
    MtProbe p;
    p.xk = __builtin_amdgcn_alignbit(w1, w2, 32 - 2 * P2);
    p.voff = (int)((w1 >> (32 - 2 * P2)) << (C16 ? 4 : 5));
    p.ra = __builtin_amdgcn_raw_buffer_load_b128(mtab, p.voff, 0, 0);
    return p;
}
// ... the other four keys only with more than two suffixes and a query key beyond the second (keys ascend) ...
template <bool C16>
__device__ __forceinline__ mt_v4i mt_second(const __amdgpu_buffer_rsrc_t mtab, const MtProbe &p)
{
    mt_v4i rb = mt_v4i{p.ra.z, p.ra.z, p.ra.z, p.ra.z};
    if (!C16 && ((uint32_t)p.ra.x >> 24) > 2u && p.xk > (uint32_t)p.ra.w) rb = __builtin_amdgcn_raw_buffer_load_b128(mtab, p.voff + 16, 0, 0);
    return rb;
}
typedef unsigned short mt_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t mt_pk_min(uint32_t a, uint32_t b)        // v_pk_min_u16
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(mt_us2, a), __builtin_bit_cast(mt_us2, b)));
}
// smallest of (key ^ xk16) over the six 16-bit keys of a compact entry's dwords 1..3; `more`: the last slot holds the
// row count, not a key
__device__ __forceinline__ uint32_t mt_xmin16(const mt_v4i e, uint32_t xk16, bool more)
{
    const uint32_t xx = xk16 * 0x10001u;
    uint32_t d3 = (uint32_t)e.w ^ xx;
    d3 |= more ? 0xFFFF0000u : 0u;
    const uint32_t mm = mt_pk_min(mt_pk_min((uint32_t)e.y ^ xx, (uint32_t)e.z ^ xx), d3);
    return min(mm & 0xFFFFu, mm >> 16);
}
__device__ __forceinline__ int mt_lcp16(uint32_t x16) { return x16 ? (__clz((int)x16) - 16) >> 1 : 8; }      // 8 when a key agrees in full
// ... and the proven match length `best0` (not yet capped by the bases left); `slow`: the entry could not decide
// (meaningful only where best0 < bases left).
template <bool C16>
__device__ __forceinline__ int mt_eval(const MtProbe &p, const mt_v4i rb, int P2, bool &slow)
{
    if (C16) {
        const uint32_t w0 = (uint32_t)p.ra.x, cnt4 = (w0 >> 24) & 15u, nib = w0 >> 28;
        const bool wide = (nib & kM16Wide) && cnt4 >= 1u && cnt4 <= 3u;         // three 16-base keys instead of six 8-base ones
        const bool rows_decide = cnt4 == kM16More || (cnt4 != 0 && !wide && (nib & kM16General));      // the entry alone only proves P2 bases
        // one evaluation for both key widths: the same three xor against the continuation (16 bases) or against its first 8 bases
        // twice over; narrow keys: the smaller half of the packed minimum, moved to the top half with ones below it, so that one
        // leading-zero count serves both (8 when a narrow key agrees in full, 16 when a wide one does).  An entry of 7 .. 13
        // suffixes keeps a row count in its last slot: it is "rows decide" below, whatever comes out here.
        const uint32_t xx = wide ? p.xk : (p.xk >> 16) * 0x10001u;
        const uint32_t d1 = (uint32_t)p.ra.y ^ xx, d2 = (uint32_t)p.ra.z ^ xx, d3 = (uint32_t)p.ra.w ^ xx;
        const uint32_t mm = mt_pk_min(mt_pk_min(d1, d2), d3);
        const uint32_t xn = (min(mm & 0xFFFFu, mm >> 16) << 16) | 0xFFFFu;
        const uint32_t xw = min(min(d1, d2), d3);
        const int lcp = __clz((int)(wide ? xw : xn)) >> 1;
        slow = cnt4 != 0 && (rows_decide || lcp == (wide ? 16 : 8));
        return cnt4 == 0 ? (int)nib : (rows_decide ? P2 : P2 + lcp);
    }
    const uint32_t meta = (uint32_t)p.ra.x;
    uint32_t x = min(p.xk ^ (uint32_t)p.ra.z, p.xk ^ (uint32_t)p.ra.w);
    x = min(x, min(min(p.xk ^ (uint32_t)rb.x, p.xk ^ (uint32_t)rb.y), min(p.xk ^ (uint32_t)rb.z, p.xk ^ (uint32_t)rb.w)));
    const int lcp = __clz((int)x) >> 1;                        // 16 when a key agrees in full
    const int lm = (int)((meta >> 8) & 0x1Fu);
    slow = (meta & kMatchSlow) || lcp + lm == 16 + 0x1F;
    return (int)(meta & 0xFFu) + (lcp & lm);
}

// Round 2 of one quad (positions a .. a+3, a % 4 == 0, m >= 2 bases left at a) whose sample v0 = fwd[a] differs
// from the next quad's sample v4 (or has none): the MIDDLE position first, then a neighbour of it only where the
// middle still leaves it open -- fwd[] is non-decreasing, so fwd[a+2] == fwd[a] settles a+1 and
// fwd[a+2] == fwd[a+4] (or == L) settles a+3.  d0..d2: the packed-read dwords that hold all three windows,
// sh = 32 - (bit offset of position a in d0) (31, 23, 15 or 7).  Outputs: absolute ends v1..v3 (0 where the position
// does not exist) and whether each still needs the slow path.
struct MtQuad {
    uint32_t v1, v2, v3;
    bool s1, s2, s3;
};
template <bool C16>
__device__ __forceinline__ MtQuad mt_quad_interior(const __amdgpu_buffer_rsrc_t mtab, int P2, uint32_t d0, uint32_t d1, uint32_t d2,
                                                   uint32_t sh, int a, int m, int L, uint32_t v0, bool has_right, uint32_t v4,
                                                   bool look_up_all)
{
    MtQuad q{v0, 0u, 0u, false, false, false};
    const int km = m > 2 ? 2 : 1;                                   // a quad cut to two positions: its second
    const MtProbe pm = mt_issue<C16>(mtab, __builtin_amdgcn_alignbit(d0, d1, sh - 2 * km), __builtin_amdgcn_alignbit(d1, d2, sh - 2 * km), P2);
    const mt_v4i rm = mt_second<C16>(mtab, pm);
    bool sm;
    const int bm = mt_eval<C16>(pm, rm, P2, sm);
    const int em = bm < m - km ? bm : m - km;
    sm = sm && m - km > bm;
    const uint32_t vm = (uint32_t)(a + km + em);
    if (km == 1) {
        q.v1 = vm;
        q.s1 = sm;
        return q;
    }
    q.v2 = vm;
    q.s2 = sm;
    const bool need1 = look_up_all || sm || vm != v0;
    const bool need3 = m > 3 && (look_up_all || sm || !((has_right && vm == v4) || (int)vm == L));
    q.v1 = v0;                                                       // == vm where it is not looked up
    q.v3 = m > 3 ? vm : 0u;                                          // == v4 or L where it is not looked up
    if (need1 || need3) {
        const uint32_t s13 = need1 ? sh - 2 : sh - 6;                 // a lane that needs both: a+1 here, a+3 below
        const MtProbe pa = mt_issue<C16>(mtab, __builtin_amdgcn_alignbit(d0, d1, s13), __builtin_amdgcn_alignbit(d1, d2, s13), P2);
        MtProbe pb = pa;
        const bool both = need1 && need3;
        if (both) pb = mt_issue<C16>(mtab, __builtin_amdgcn_alignbit(d0, d1, sh - 6), __builtin_amdgcn_alignbit(d1, d2, sh - 6), P2);
        const mt_v4i ra = mt_second<C16>(mtab, pa);
        mt_v4i rb = ra;
        if (both) rb = mt_second<C16>(mtab, pb);
        bool sa, sb;
        const int ba = mt_eval<C16>(pa, ra, P2, sa), bb = mt_eval<C16>(pb, rb, P2, sb);
        const int ka = need1 ? 1 : 3;
        const int ea = ba < m - ka ? ba : m - ka, eb = bb < m - 3 ? bb : m - 3;
        sa = sa && m - ka > ba;
        sb = sb && m - 3 > bb;
        if (need1) { q.v1 = (uint32_t)(a + 1 + ea); q.s1 = sa; }
        else { q.v3 = (uint32_t)(a + 3 + ea); q.s3 = sa; }
        if (both) { q.v3 = (uint32_t)(a + 3 + eb); q.s3 = sb; }
    }
    return q;
}

// Slow path over list[c0 .. c0 + 64): positions whose table entry could not decide.
//   LONG = false: entries are (read << 8 | position) of a group of short reads, results go to their byte rows;
//   LONG = true:  one long read of L0 bases; entries are positions relative to `wbase` (the window being worked
//                 on), results go to the window's row `fwW` (uint16; int32 for genie_find_smems_long).
// QB: how the packed read is read -- QBits over Dp (LDS), or QPlain over plain 64-bit words (LONG only: Dp then points
// at the words of the read).
template <bool LONG, bool C16, class QB = QBits, class FW = uint16_t>
__device__ __forceinline__ void mt_slow(const DevIndex &ix, const __amdgpu_buffer_rsrc_t mtab, const __amdgpu_buffer_rsrc_t ov, int mode, int lane, int c0,
                                        int count, const uint16_t *list, const uint32_t *Dp, int DW, const int *Ls,
                                        uint8_t *fwL, int FS, int L0 = 0, int wbase = 0, FW *fwW = nullptr)
{
    const int K = ix.K, P = ix.P, P2 = ix.P2;
    const int idx = c0 + lane;
    const bool on = idx < count;
    int u = 0, a = 0, m = 0, best = 0, chain = 0, cvoff = 0, nrows = 0;
    uint32_t mask = 0, lb = 0, c = 0, xmin = ~0u, xkq = 0;
    bool general = false;
    uint64_t w = 0, xq = 0;
    QB Q{reinterpret_cast<decltype(QB::p)>(Dp)};
    if (on) {
        const uint32_t e = (uint32_t)list[idx];
        if constexpr (LONG) {
            a = wbase + (int)e;
            m = L0 - a;
        } else {
            u = (int)(e >> 8);
            a = (int)(e & 255u);
            m = Ls[u] - a;
            Q.p = Dp + u * DW;
        }
        w = Q.win(a);
        xq = Q.win(a + P);
        c = (uint32_t)(w >> (64 - 2 * P2));
        const uint32_t xk = (uint32_t)((w << (2 * P2)) >> 32);
        if (C16) {
            // compact entry: six 8-base keys inline (three 16-base ones in a wide-key entry; five + an overflow block of eight for 7 .. 13 suffixes)
            const mt_v4i e = __builtin_amdgcn_raw_buffer_load_b128(mtab, (int)(c << 4), 0, 0);
            const uint32_t w0 = (uint32_t)e.x, cnt4 = (w0 >> 24) & 15u, xk16 = xk >> 16;
            lb = w0 & 0xFFFFFFu;
            best = P2;
            const uint32_t total = cnt4 == kM16More ? 7u + (w0 >> 28) : cnt4;
            const bool wide = ((w0 >> 28) & kM16Wide) && cnt4 >= 1u && cnt4 <= 3u;
            general = cnt4 != kM16More && !wide && ((w0 >> 28) & kM16General) != 0;
            nrows = (int)total;
            if (wide) {
                const uint32_t k32[3] = {(uint32_t)e.y, (uint32_t)e.z, (uint32_t)e.w};
                uint32_t xm = ~0u;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    xm = min(xm, k32[i] ^ xk);
                    mask |= (k32[i] == xk && (uint32_t)i < cnt4) ? 1u << i : 0u;
                }
                const int lcp = __clz((int)xm) >> 1;
                const int l = P2 + lcp < m ? P2 + lcp : m;
                best = l > best ? l : best;
                if (lcp < 16 || m <= P2 + 16) mask = 0;                        // decided without the rows
            } else if (!general) {
                const uint32_t k16[6] = {(uint32_t)e.y & 0xFFFFu, (uint32_t)e.y >> 16, (uint32_t)e.z & 0xFFFFu,
                                         (uint32_t)e.z >> 16, (uint32_t)e.w & 0xFFFFu, (uint32_t)e.w >> 16};
                const uint32_t ninl = cnt4 == kM16More ? (uint32_t)kM16Keys - 1u : cnt4;
#pragma unroll
                for (int i = 0; i < kM16Keys; i++) mask |= (k16[i] == xk16 && (uint32_t)i < ninl) ? 1u << i : 0u;
                uint32_t xm = mt_xmin16(e, xk16, cnt4 == kM16More);
                if (cnt4 == kM16More) mt_ov_scan(ov, (uint32_t)e.w >> 16, (int)total - (kM16Keys - 1), xk16, 0xFFFFu, xm, mask);
                const int lcp = mt_lcp16(xm);
                const int l = P2 + lcp < m ? P2 + lcp : m;
                best = l > best ? l : best;
                if (lcp < 8 || m <= P2 + 8) mask = 0;                          // decided without the rows
            }
        }
        if (!C16) {
            const mt_v4i ra = __builtin_amdgcn_raw_buffer_load_b128(mtab, (int)(c << 5), 0, 0);
            const mt_v4i rb = __builtin_amdgcn_raw_buffer_load_b128(mtab, (int)(c << 5) + 16, 0, 0);
            const uint32_t meta = (uint32_t)ra.x;
            lb = (uint32_t)ra.y;                                               // first row of the P2-mer
            best = P2;
            general = (meta & (kMatchSlow | kMatchMore)) == kMatchSlow;
            const uint32_t rows = meta >> 24;
            nrows = (int)rows;
            if (!general) {
                mask = ((uint32_t)ra.z == xk ? 1u : 0u) | ((uint32_t)ra.w == xk ? 2u : 0u) | ((uint32_t)rb.x == xk ? 4u : 0u) |
                       ((uint32_t)rb.y == xk ? 8u : 0u) | ((uint32_t)rb.z == xk ? 16u : 0u);
                if (meta & kMatchMore) {
                    // kMatchKeys - 1 keys here, the others eight per overflow entry: the fast path proved only P2 bases
                    chain = (int)((rows - (kMatchKeys - 1) + 7) >> 3);
                    cvoff = (int)((uint32_t)rb.w << 5);
                    xmin = min(min(xk ^ (uint32_t)ra.z, xk ^ (uint32_t)ra.w), min(min(xk ^ (uint32_t)rb.x, xk ^ (uint32_t)rb.y), xk ^ (uint32_t)rb.z));
                } else {
                    mask |= (uint32_t)rb.w == xk ? 32u : 0u;
                    mask &= (1u << rows) - 1u;                                 // unused slots repeat key[0]
                }
            }
        }
        xkq = xk;
    }
    // chained entries: the rest of the keys (ascending, unused slots repeat the first key of the chain's bucket)
    for (int e = 0; __any(e < chain); e++) {
        if (e < chain) {
            const mt_v4i ca = __builtin_amdgcn_raw_buffer_load_b128(mtab, cvoff + 32 * e, 0, 0);
            const mt_v4i cb = __builtin_amdgcn_raw_buffer_load_b128(mtab, cvoff + 32 * e + 16, 0, 0);
            const uint32_t k8[8] = {(uint32_t)ca.x, (uint32_t)ca.y, (uint32_t)ca.z, (uint32_t)ca.w, (uint32_t)cb.x, (uint32_t)cb.y, (uint32_t)cb.z, (uint32_t)cb.w};
            uint32_t eq = 0;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                xmin = min(xmin, xkq ^ k8[i]);
                eq |= k8[i] == xkq ? 1u << i : 0u;
            }
            mask |= eq << (kMatchKeys - 1 + 8 * e);
        }
    }
    if (chain) {
        // what the whole chain proves; rows past the bucket (filler slots) cannot agree unless the first key does
        const int lcp = __clz((int)xmin) >> 1;
        const int l = P2 + lcp < m ? P2 + lcp : m;
        best = l > best ? l : best;
        if (lcp < 16 || m <= P2 + 16) mask = 0;                               // decided without the rows
        else mask &= nrows >= 32 ? ~0u : (1u << nrows) - 1u;
    }
    // rows whose 16-base key agrees: the longest match is the longest of theirs
    while (__any(mask != 0)) {
        if (mask) {
            const int i = __ffs((int)mask) - 1;
            mask &= mask - 1;
            const Cmp r = cmp_rec(ix, Q, a, m, load_rec(ix.sa, (int)lb + i), xq);
            best = r.l > best ? r.l : best;
        }
    }
    if (__any(general)) {
        int lo = 0, hi = 0, hint = -1;
        if (general) {
            int4 hd = *reinterpret_cast<const int4 *>(ix.dir2 + c);
            asm volatile("" : "+v"(hd.x), "+v"(hd.y), "+v"(hd.z), "+v"(hd.w));
            const uint32_t cnt = (uint32_t)hd.y & ~kHeadShort;
            lo = hd.x;
            hi = hd.x + (int)cnt;
            const uint64_t key = ((uint64_t)(uint32_t)hd.w << 32) | (uint32_t)hd.z;
            const uint64_t x = xq ^ key;
            // the first row's key copy decides whenever the comparison ends inside the key
            if (!((uint32_t)hd.y & kHeadShort) && (x != 0 || m <= P + 32)) {
                int l = x ? P + (__clzll((long long)x) >> 1) : m;
                bool less = key < xq;
                if (l >= m) { l = m; less = false; }
                best = l > best ? l : best;
                if (less) lo = hd.x + 1; else hi = hd.x;
            }
            if (mode == GENIE_MODE_RMI && m >= K && K >= P2) {
                const double p = rmi_predict(ix, nullptr, 0, (uint32_t)(w >> (64 - 2 * K)));
                hint = !(p > 0.0) ? 0 : (p >= (double)ix.n ? ix.n : (int)p);              // int(start_sa)
            }
        }
        while (__any(lo < hi)) {
            if (lo < hi) {
                int mid = (lo + hi) >> 1;
                if (hint >= lo && hint < hi) mid = hint;
                hint = -1;
                const Cmp r = cmp_rec(ix, Q, a, m, load_rec(ix.sa, mid), xq);
                best = r.l > best ? r.l : best;
                if (r.less) lo = mid + 1; else hi = mid;
            }
        }
    }
    if (on) {
        if (LONG) fwW[a - wbase] = (FW)(a + best);
        else fwL[u * FS + a] = (uint8_t)(a + best);
    }
}

// PK: the reads arrive 2-bit packed (genie_find_smems_packed: byte i of a row = bases 4i .. 4i+3, the first in bits 7..6),
// so the pack stage is one dword load and a byte swap per 16 bases, and no base can be invalid.
template <int WPS, bool C16, bool PK>
__global__ void __launch_bounds__(512, WPS) match_table_kernel(DevIndex ix, int mode, const uint8_t *__restrict__ reads,
                                                             const int32_t *__restrict__ lens, long long N, int stride,
                                                             int fixed_len, uint8_t *__restrict__ fwd_out, int fwd_stride,
                                                             RefRec *__restrict__ qp_out, int qp_recs, int qp_stride,
                                                             int32_t *__restrict__ status, int grp, int max_len,
                                                             long long mtab_bytes, int flags, int cus)
{
    typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
    extern __shared__ __align__(16) uint8_t smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const int waves_per_block = blockDim.x >> 6;
    const int dbg = (flags >> 8) & 63;                            // experiments only (GENIE_OPT_SEARCH_ONLY): stages off
    const int sched = flags >> 16;                                // GENIE_OPT_SCHEDULING (A/B timing)
    const bool look_up_all = (flags & 1) != 0;                    // GENIE_OPT_SEARCH_ALL: no sampling
    const int FS = fwd_stride;
    const int K = ix.K;
    const int P2 = ix.P2;
    const int DW = mt_short_row_dwords(max_len, qp_recs);         // dwords per packed read in LDS
    const int DWp = mt_pack_dwords(max_len);                      // of which the first DWp are rewritten per iteration
    const int QL = mt_quads(max_len);                             // quads per read
    const int nquads = grp * QL;
    const __amdgpu_buffer_rsrc_t mtab =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<MatchRec *>(ix.mtab), 0, (int)mtab_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ov =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<MatchOv16 *>(ix.ov), 0, ix.ov_entries * (int)sizeof(MatchOv16), 0x00020000);

    uint8_t *wb = smem + wave * mt_wave_bytes(grp, max_len, qp_recs, FS);
    uint32_t *Dp = reinterpret_cast<uint32_t *>(wb);
    int *Ls = reinterpret_cast<int *>(wb + mt_r16(grp * DW * 4));                                  // kMtMaxG
    uint8_t *fwL = reinterpret_cast<uint8_t *>(Ls) + 64;
    uint16_t *sl = reinterpret_cast<uint16_t *>(fwL + mt_r16(grp * FS));
    uint16_t *qa = reinterpret_cast<uint16_t *>(reinterpret_cast<uint8_t *>(sl) + mt_r16(grp * max_len * 2));
    uint16_t *qb = qa + grp * mt_quads(max_len);
    for (int i = lane; i < grp * DW; i += kWave) Dp[i] = 0;                    // the zero padding behind every read
    const uint8_t *reads_end = reads + N * (long long)stride;

    // lane t of the pack pass: dword j of read u
    const int pu = (int)(((uint32_t)lane * (uint32_t)(65536 / DWp + 1)) >> 16);    // lane / DWp, exact below 64
    const int pj = lane - pu * DWp;

    // Who works on which group of reads, and when.  (1) A block owns a contiguous share of the groups and its waves take them one
    // at a time from a counter in LDS: groups differ in work (lookups, slow-path items).  (2) A CU issues for its OLDEST waves
    // first, so of the three blocks of a CU the first to arrive ran ahead and the last fell behind: with equal shares the blocks of
    // the first, second and third round of the launch finished at 0.39, 0.45 and 0.54 ms of a 0.55 ms kernel, the CU's last
    // third running on a third of its waves.  Every wave therefore changes its issue priority with every group it starts
    // (s_setprio; the level a function of the group count and of the round its block belongs to), which shares the CU evenly:
    // 0.53 -> 0.48 ms per 10^6 reads on the 100 kb reference, 3.49 -> 3.42 ms per 4 x 10^6 on the 1 Mb one (tools/experiments/README.md).
    // (A counter in global memory instead -- one for the grid, or one per block with stealing -- cost 4 to 16 times the kernel's
    // time: returning device-scope atomics are slow here, and every later load of the wave waits behind them.)
    uint32_t *next_group = reinterpret_cast<uint32_t *>(smem + waves_per_block * mt_wave_bytes(grp, max_len, qp_recs, FS));
    const long long groups = (N + grp - 1) / grp;
    const long long share = (groups + gridDim.x - 1) / gridDim.x;
    const long long g_begin = (long long)blockIdx.x * share;
    const long long g_end = g_begin + share < groups ? g_begin + share : groups;
    const bool handed_out = !(sched & 1), rotate = !(sched & 2);
    if (threadIdx.x == 0) *next_group = (uint32_t)waves_per_block;
    // quad t of a group: x = read << 28 | byte offset of its sample in the fwd rows << 16 | position; y = dword offset of its
    // window in the packed reads << 8 | the window's shift.  (Worked out per lookup these were a dozen instructions of the ~80
    // a lookup costs; the kernel is bound by instruction issue on a table that fits the L2.)
    uint2 *qtab = reinterpret_cast<uint2 *>(next_group + 4);
    for (int t = threadIdx.x; t < (nquads + 191) / 192 * 192; t += blockDim.x) {
        const int tq = t < nquads ? t : 0;
        const int u = tq / QL, a = 4 * (tq - u * QL);
        const uint32_t o = 2u * (uint32_t)a + 1u;
        qtab[t] = make_uint2((uint32_t)u << 28 | (uint32_t)(u * FS + a) << 16 | (uint32_t)a,
                             ((uint32_t)(u * DW) + (o >> 5)) << 8 | (32u - (o & 31u)));
    }
    __syncthreads();
    long long gi = handed_out ? g_begin + wave : (long long)blockIdx.x * waves_per_block + wave;
    const long long g_stop = handed_out ? g_end : groups;
    const int round_of_block = (int)(blockIdx.x / (uint32_t)cus);
    const bool touch_ahead = !(sched & 8);
    for (int it = 0; gi < g_stop; it++) {
        const long long r = gi * grp;
        if (rotate) set_wave_priority(it + round_of_block);
        // the group after this one is claimed NOW, so that its input rows can be asked for through the scalar cache while this
        // group is worked on: they come from HBM, and a line from there keeps the CU's L1 busy seven to nine times as long as a
        // table entry does (scalar_touch_lines, kernels.hip)
        long long gi_next;
        if (handed_out) {
            uint32_t nx = 0;
            if (lane == 0) nx = atomicAdd(next_group, 1u);
            gi_next = g_begin + (long long)(uint32_t)rfl((int)nx);
        } else {
            gi_next = gi + (long long)gridDim.x * waves_per_block;
        }
        if (touch_ahead && stride > 0 && gi_next < g_stop) {
            const long long rn = gi_next * grp;
            const long long rows = N - rn < (long long)grp ? N - rn : (long long)grp;
            scalar_touch_lines(reads + rn * (long long)stride, (uint32_t)(rows * stride));
        }
        // ---- pack: one pass per 64 / DWp reads
        bool any_read = false;
        for (int u0 = 0; u0 < grp; u0 += kWave / DWp) {
            const int u = u0 + pu;
            const bool mine = pu < kWave / DWp && u < grp;
            int L = 0, st = GENIE_READ_OK;
            uint32_t d = 0;
            bool bad = false;
            if (mine && r + u < N) {
                L = lens ? lens[r + u] : fixed_len;
                if (L < 0 || L > max_len) { st = GENIE_READ_BAD_BASE; L = 0; }       // host validates lengths; defensive only
                const int left = L - 16 * pj;
                if (PK) {
                    if (left > 0) {
                        d = __builtin_bswap32(*reinterpret_cast<const uint32_t *>(reads + (r + u) * (long long)stride + 4 * pj));
                        if (left < 16) d &= ~0u << (32 - 2 * left);                 // whatever lies behind the read is not part of it
                    }
                }
                const uint8_t *src = reads + (r + u) * (long long)stride + 16 * pj;
                uint32_t v[4] = {0, 0, 0, 0};
                if (PK) {
                } else if (left >= 16 || (left > 0 && src + 16 <= reads_end)) {
                    // ONE 16-byte load (rows start at any byte: the hardware's unaligned mode serves it; four dword loads
                    // were four L1 requests for the same lines).  A read's last, partial piece is loaded whole as well --
                    // what lies behind it is the next read's row -- and cut to its length; only the piece at the very end of
                    // the input takes the byte loads below.
                    const nt_u4 q = *reinterpret_cast<const nt_u4_unaligned *>(src);
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                    if (left < 16) {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const int nb = left - 4 * k;                          // bytes of dword k that belong to the read
                            v[k] = nb >= 4 ? v[k] : (nb <= 0 ? 0u : v[k] & ((1u << (8 * nb)) - 1u));
                        }
                    }
                } else if (left > 0) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (left >= 4 * k + 4) v[k] = *reinterpret_cast<const u32_unaligned *>(src + 4 * k);
                        else for (int b = 0; b < left - 4 * k; b++) v[k] |= (uint32_t)src[4 * k + b] << (8 * b);
                    }
                }
                if (!PK) {
                    bad = ((v[0] | v[1] | v[2] | v[3]) & 0xFCFCFCFCu) != 0;
                    d = (mt_pack4(v[0]) << 24) | (mt_pack4(v[1]) << 16) | (mt_pack4(v[2]) << 8) | mt_pack4(v[3]);
                }
            }
            // the stream one bit to the right: bit 31 comes from the dword before (lane - 1; a read's first dword
            // gets a stray pad bit that no window ever covers)
            const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)d, 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
            const unsigned long long badm = __ballot(bad);
            bool ok = false;
            if (mine) {
                Dp[u * DW + pj] = __builtin_amdgcn_alignbit(prev, d, 1);
                if (pj == 0) {
                    const unsigned long long mine_bits = ((1ull << DWp) - 1ull) << (pu * DWp);
                    if (st == GENIE_READ_OK && (badm & mine_bits)) st = GENIE_READ_BAD_BASE;
                    if (st == GENIE_READ_OK && mode != GENIE_MODE_BWA && L < K) st = GENIE_READ_TOO_SHORT;
                    if (r + u < N) status[r + u] = st;
                    ok = st == GENIE_READ_OK && L > 0;
                    Ls[u] = ok ? L : 0;
                }
            }
            any_read |= __any(ok);
        }
        wave_lds_fence();
        if (any_read) {
            // the packed read for K_C, as plain 64-bit words (zeros behind the read): piece i of a read = its words 2i and 2i + 1.
            // (Until round 3 these were overlapping records {w[i], w[i+1]}, twice the bytes, so that a window was one ALIGNED
            // 16-byte load; K_C takes its windows with 8-byte-aligned 16-byte loads now and a read's slot is 80 bytes instead of
            // 128 at 150 bases -- the lines K_C streams from HBM are what fills its vector-miss slots, DESIGN.md section 4.)
            for (int t0 = 0; t0 < ((dbg & 8) ? 0 : grp * qp_recs); t0 += kWave) {
                const int t = t0 + lane;
                const int u = t / qp_recs, i = t - u * qp_recs;
                if (t < grp * qp_recs && Ls[u] > 0) {
                    const uint32_t *q = Dp + u * DW + 4 * i;
                    const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
                    uint4 rec;                                  // un-shifted dwords 4i .. 4i+3, low dword of each word first
                    rec.y = __builtin_amdgcn_alignbit(q0, q1, 31);
                    rec.x = __builtin_amdgcn_alignbit(q1, q2, 31);
                    rec.w = __builtin_amdgcn_alignbit(q2, q3, 31);
                    rec.z = __builtin_amdgcn_alignbit(q3, q4, 31);
                    store_nt(qp_out + (r + u) * (long long)qp_stride + i, rec);
                }
            }
            // ---- round 1: the first position of every quad
            int nslow = 0;
#pragma nounroll
            for (int c0 = 0; c0 < ((dbg & 4) ? 0 : nquads); c0 += kMtNsp * kWave) {
                uint32_t ent[kMtNsp];                             // read << 28 | fwd-row byte offset << 16 | bases left << 8 | position
                MtProbe pr[kMtNsp];
#pragma unroll
                for (int s = 0; s < kMtNsp; s++) {
                    const int t0 = c0 + 64 * s + lane;
                    const uint2 q = qtab[t0];                     // idle lanes look up quad 0 and drop the result
                    int m = Ls[q.x >> 28] - (int)(q.x & 255u);
                    m = t0 < nquads && m > 0 ? m : 0;
                    ent[s] = q.x | ((uint32_t)m << 8);
                    const uint32_t *dq = Dp + (q.y >> 8);
                    const uint32_t sh = q.y & 255u;
                    const uint32_t d0 = dq[0], d1 = dq[1], d2 = dq[2];
                    pr[s] = mt_issue<C16>(mtab, __builtin_amdgcn_alignbit(d0, d1, sh), __builtin_amdgcn_alignbit(d1, d2, sh), P2);
                }
                mt_v4i rb[kMtNsp];
#pragma unroll
                for (int s = 0; s < kMtNsp; s++) rb[s] = mt_second<C16>(mtab, pr[s]);
#pragma unroll
                for (int s = 0; s < kMtNsp; s++) {
                    bool slow;
                    const int best0 = mt_eval<C16>(pr[s], rb[s], P2, slow);
                    const int a = (int)(ent[s] & 255u), m = (int)((ent[s] >> 8) & 255u);
                    const int best = best0 < m ? best0 : m;
                    if (m) fwL[(ent[s] >> 16) & 0xFFFu] = (uint8_t)(a + best);
                    slow = slow && m > best0;
                    const unsigned long long sb = __ballot(slow);
                    if (slow) sl[nslow + __popcll(sb & ((1ull << lane) - 1ull))] = (uint16_t)(((ent[s] >> 28) << 8) | (uint32_t)a);
                    nslow += __popcll(sb);
                }
            }
            wave_lds_fence();
#pragma nounroll
            for (int c0 = 0; c0 < ((dbg & 1) ? 0 : nslow); c0 += kWave) mt_slow<false, C16>(ix, mtab, ov, mode, lane, c0, nslow, sl, Dp, DW, Ls, fwL, FS);
            wave_lds_fence();
            // ---- round 2: the other three positions of a quad, looked up only where the quad's sample and the next
            // quad's differ (and the match does not already reach the end of the read): the MIDDLE position first, a
            // neighbour only where the middle leaves it open (fwd[] is non-decreasing: fwd[a+2] == fwd[a] settles a+1,
            // fwd[a+2] == fwd[a+4] or == L settles a+3).  Three passes, each over a DENSE list, so that every lane of a
            // lookup pass has work (a lane per quad with two dependent lookups inside ran at a third of the lanes and
            // three times the instructions per lookup of round 1): the quads to work on, their middles, the neighbours.
            nslow = 0;
            int nqa = 0, nqb = 0;
            const unsigned long long below = (1ull << lane) - 1ull;
#pragma nounroll
            for (int t0 = lane; t0 < ((dbg & 6) ? 0 : nquads) + lane; t0 += kWave) {           // uniform trip count (ballots inside)
                const uint2 q = qtab[t0 < nquads ? t0 : 0];
                const int u = (int)(q.x >> 28), a = (int)(q.x & 255u);
                const int L = Ls[u];
                const int m = t0 < nquads && L > a ? L - a : 0;
                const uint32_t fo = (q.x >> 16) & 0xFFFu;
                const uint32_t v0 = fwL[fo];
                const bool has_right = m > 4;
                const uint32_t v4 = has_right ? fwL[fo + 4] : 0u;
                const bool need = m > 1 && (look_up_all || ((int)v0 != L && !(has_right && v4 == v0)));
                if (m && !need) *reinterpret_cast<uint32_t *>(fwL + fo) = v0 * 0x01010101u;       // the quad shares its sample's value
                const unsigned long long nb = __ballot(need);
                if (need) qa[nqa + __popcll(nb & below)] = (uint16_t)((uint32_t)u << 8 | (uint32_t)a);
                nqa += __popcll(nb);
            }
            wave_lds_fence();
            // the middles (position a + 2; a + 1 in a quad cut to two positions).  One lookup per lane and pass: the
            // CU's miss queue is full with a fraction of its waves' requests anyway.
#pragma nounroll
            for (int c0 = 0; c0 < nqa; c0 += kWave) {
                const bool valid = c0 + lane < nqa;
                const uint32_t it = qa[valid ? c0 + lane : 0];
                const int u = (int)(it >> 8), a = (int)(it & 255u);
                const int L = Ls[u], m = L - a;                    // m > 1: the quad is on the list
                const int km = m > 2 ? 2 : 1;
                const uint32_t fo = __umul24((uint32_t)u, (uint32_t)FS) + (uint32_t)a;
                const uint32_t o = 2u * (uint32_t)(a + km) + 1u;
                const uint32_t *dq = Dp + __umul24((uint32_t)u, (uint32_t)DW) + (o >> 5);
                const uint32_t sh = 32u - (o & 31u);
                const uint32_t d0 = dq[0], d1 = dq[1], d2 = dq[2];
                const MtProbe pm = mt_issue<C16>(mtab, __builtin_amdgcn_alignbit(d0, d1, sh), __builtin_amdgcn_alignbit(d1, d2, sh), P2);
                const uint32_t v0 = fwL[fo];
                const bool has_right = m > 4;
                const uint32_t v4 = has_right ? fwL[fo + 4] : 0u;
                const mt_v4i rm = mt_second<C16>(mtab, pm);
                bool sm;
                const int bm = mt_eval<C16>(pm, rm, P2, sm);
                const int em = bm < m - km ? bm : m - km;
                sm = valid && sm && m - km > bm;
                const uint32_t vm = (uint32_t)(a + km + em);
                bool need1 = false, need3 = false;
                if (valid) {
                    if (km == 1) {
                        *reinterpret_cast<uint32_t *>(fwL + fo) = v0 | vm << 8;
                    } else {
                        need1 = look_up_all || sm || vm != v0;
                        need3 = m > 3 && (look_up_all || sm || !((has_right && vm == v4) || (int)vm == L));
                        // a + 1 == the sample's value and a + 3 == the middle's wherever they are not looked up
                        *reinterpret_cast<uint32_t *>(fwL + fo) = v0 | v0 << 8 | vm << 16 | (m > 3 ? vm : 0u) << 24;
                    }
                }
                const unsigned long long sbm = __ballot(sm), b1 = __ballot(need1), b3 = __ballot(need3);
                if (sm) sl[nslow + __popcll(sbm & below)] = (uint16_t)(it + (uint32_t)km);
                nslow += __popcll(sbm);
                if (need1) qb[nqb + __popcll(b1 & below)] = (uint16_t)(it + 1u);
                nqb += __popcll(b1);
                if (need3) qb[nqb + __popcll(b3 & below)] = (uint16_t)(it + 3u);
                nqb += __popcll(b3);
            }
            wave_lds_fence();
            // the neighbours (positions a + 1 and a + 3) that the middles left open
#pragma nounroll
            for (int c0 = 0; c0 < nqb; c0 += kWave) {
                const bool valid = c0 + lane < nqb;
                const uint32_t it = qb[valid ? c0 + lane : 0];
                const int u = (int)(it >> 8), a = (int)(it & 255u);
                const int m = Ls[u] - a;                           // >= 1
                const uint32_t o = 2u * (uint32_t)a + 1u;
                const uint32_t *dq = Dp + __umul24((uint32_t)u, (uint32_t)DW) + (o >> 5);
                const uint32_t sh = 32u - (o & 31u);
                const uint32_t d0 = dq[0], d1 = dq[1], d2 = dq[2];
                const MtProbe pn = mt_issue<C16>(mtab, __builtin_amdgcn_alignbit(d0, d1, sh), __builtin_amdgcn_alignbit(d1, d2, sh), P2);
                const mt_v4i rn = mt_second<C16>(mtab, pn);
                bool slow;
                const int b0 = mt_eval<C16>(pn, rn, P2, slow);
                const int e = b0 < m ? b0 : m;
                if (valid) fwL[__umul24((uint32_t)u, (uint32_t)FS) + (uint32_t)a] = (uint8_t)(a + e);
                slow = valid && slow && m > b0;
                const unsigned long long sb = __ballot(slow);
                if (slow) sl[nslow + __popcll(sb & below)] = (uint16_t)it;
                nslow += __popcll(sb);
            }
            wave_lds_fence();
#pragma nounroll
            for (int c0 = 0; c0 < ((dbg & 1) ? 0 : nslow); c0 += kWave) mt_slow<false, C16>(ix, mtab, ov, mode, lane, c0, nslow, sl, Dp, DW, Ls, fwL, FS);
            wave_lds_fence();
            // ---- results: fwd rows
            const int nrows = N - r < (long long)grp ? (int)(N - r) : grp;
            uint4 *dst = reinterpret_cast<uint4 *>(fwd_out + r * (long long)FS);                  // rows are multiples of 16 bytes
            const uint4 *src = reinterpret_cast<const uint4 *>(fwL);
            for (int i = lane; i < ((dbg & 32) ? 0 : nrows * (FS >> 4)); i += kWave) store_nt(dst + i, src[i]);
        }
        wave_lds_fence();
        gi = gi_next;
    }
}

// ------------------------------------------------------------------ long reads (256 .. 8192 bases)
// One wave per read.  The packed read stays whole in LDS; positions are worked through in windows of kMtWinQuads
// quads whose uint16 fwd row and slow list live in LDS and go out window by window.  A window's
// round 1 also samples the first position of the NEXT window, so that its last quad has a right neighbour.
constexpr int kMtWinQuads = 176;                 // 704 positions; + 1 boundary sample <= 3 x 64 lookups of round 1
constexpr int kMtWinPos = 4 * kMtWinQuads;

__host__ __device__ inline int mt_long_wave_bytes(int max_len, int qp_recs)
{
    return mt_r16(mt_row_dwords(max_len, qp_recs) * 4) + mt_r16((kMtWinPos + 8) * 2) + mt_r16(kMtWinPos * 2);
}

template <bool C16>
__global__ void __launch_bounds__(512, 8) match_table_long_kernel(DevIndex ix, int mode, const uint8_t *__restrict__ reads,
                                                                  const int32_t *__restrict__ lens, long long N, int stride,
                                                                  int fixed_len, uint8_t *__restrict__ fwd_out, int fwd_stride,
                                                                  RefRec *__restrict__ qp_out, int qp_recs,
                                                                  int32_t *__restrict__ status, int max_len, long long mtab_bytes,
                                                                  int flags, int cus)
{
    typedef uint32_t __attribute__((aligned(1))) u32_unaligned;
    extern __shared__ __align__(16) uint8_t smem[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const int waves_per_block = blockDim.x >> 6;
    const int K = ix.K;
    const int P2 = ix.P2;
    const int DW = mt_row_dwords(max_len, qp_recs);
    const __amdgpu_buffer_rsrc_t mtab =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<MatchRec *>(ix.mtab), 0, (int)mtab_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ov =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<MatchOv16 *>(ix.ov), 0, ix.ov_entries * (int)sizeof(MatchOv16), 0x00020000);

    uint8_t *wb = smem + wave * mt_long_wave_bytes(max_len, qp_recs);
    uint32_t *Dp = reinterpret_cast<uint32_t *>(wb);
    uint16_t *fwW = reinterpret_cast<uint16_t *>(wb + mt_r16(DW * 4));
    uint16_t *sl = reinterpret_cast<uint16_t *>(reinterpret_cast<uint8_t *>(fwW) + mt_r16((kMtWinPos + 8) * 2));

    // reads handed out per block and the issue priority rotated per read, as in match_table_kernel
    const int sched = flags >> 16;
    const bool handed_out = !(sched & 1), rotate = !(sched & 2);
    uint32_t *next_read = reinterpret_cast<uint32_t *>(smem + waves_per_block * mt_long_wave_bytes(max_len, qp_recs));
    const long long share = (N + gridDim.x - 1) / gridDim.x;
    const long long r_begin = (long long)blockIdx.x * share;
    const long long r_stop = !handed_out ? N : (r_begin + share < N ? r_begin + share : N);
    if (threadIdx.x == 0) *next_read = (uint32_t)waves_per_block;
    __syncthreads();
    const int round_of_block = (int)(blockIdx.x / (uint32_t)cus);
    long long r = handed_out ? r_begin + wave : (long long)blockIdx.x * waves_per_block + wave;
    const bool touch_ahead = !(sched & 8);
    for (int it = 0; r < r_stop; it++) {
        if (rotate) set_wave_priority(it + round_of_block);
        // the next read is claimed now and its input row asked for through the scalar cache, as in match_table_kernel
        long long r_next;
        if (handed_out) {
            uint32_t nx = 0;
            if (lane == 0) nx = atomicAdd(next_read, 1u);
            r_next = r_begin + (long long)(uint32_t)rfl((int)nx);
        } else {
            r_next = r + (long long)gridDim.x * waves_per_block;
        }
        // (rows of up to 4 KB: -4 % at 500 bases, -3 % at 2000; an 8000-base row is 125 lines in one burst and cost 4 %)
        if (touch_ahead && stride > 0 && stride <= 4096 && r_next < r_stop) scalar_touch_lines(reads + r_next * (long long)stride, (uint32_t)stride);
        int L = lens ? lens[r] : fixed_len;
        int st = GENIE_READ_OK;
        if (L < 0 || L > max_len) { st = GENIE_READ_BAD_BASE; L = 0; }         // host validates lengths; defensive only
        // ---- pack: 64 dwords (1024 bases) per pass; every dword of the row is rewritten (zeros behind the read)
        {
            const uint8_t *base = reads + r * (long long)stride;
            bool bad = false;
            uint32_t carry = 0;                                                // the dword before this pass's first
            for (int j0 = 0; j0 < DW; j0 += kWave) {
                const int j = j0 + lane;
                const int left = L - 16 * j;
                uint32_t v[4] = {0, 0, 0, 0};
                if (left >= 16) {
#pragma unroll
                    for (int k = 0; k < 4; k++) v[k] = *reinterpret_cast<const u32_unaligned *>(base + 16 * j + 4 * k);
                } else if (left > 0) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (left >= 4 * k + 4) v[k] = *reinterpret_cast<const u32_unaligned *>(base + 16 * j + 4 * k);
                        else for (int b = 0; b < left - 4 * k; b++) v[k] |= (uint32_t)base[16 * j + 4 * k + b] << (8 * b);
                    }
                }
                bad |= ((v[0] | v[1] | v[2] | v[3]) & 0xFCFCFCFCu) != 0;
                const uint32_t d = (mt_pack4(v[0]) << 24) | (mt_pack4(v[1]) << 16) | (mt_pack4(v[2]) << 8) | mt_pack4(v[3]);
                uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)d, 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
                if (lane == 0) prev = carry;
                carry = (uint32_t)__builtin_amdgcn_readlane((int)d, 63);
                if (j < DW) Dp[j] = __builtin_amdgcn_alignbit(prev, d, 1);
            }
            if (__any(bad)) st = GENIE_READ_BAD_BASE;
            else if (st == GENIE_READ_OK && mode != GENIE_MODE_BWA && L < K) st = GENIE_READ_TOO_SHORT;
        }
        if (lane == 0) status[r] = st;
        wave_lds_fence();
        if (st == GENIE_READ_OK && L > 0) {
            for (int i = lane; i < qp_recs; i += kWave) {
                const uint32_t *q = Dp + 2 * i;
                const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
                uint4 rec;
                rec.y = __builtin_amdgcn_alignbit(q0, q1, 31);
                rec.x = __builtin_amdgcn_alignbit(q1, q2, 31);
                rec.w = __builtin_amdgcn_alignbit(q2, q3, 31);
                rec.z = __builtin_amdgcn_alignbit(q3, q4, 31);
                *reinterpret_cast<uint4 *>(qp_out + r * (long long)qp_recs + i) = rec;
            }
            uint16_t *frow = reinterpret_cast<uint16_t *>(fwd_out + r * (long long)fwd_stride);
#pragma nounroll
            for (int w0 = 0; w0 < L; w0 += kMtWinPos) {
                const int nq = L - w0 < kMtWinPos ? (L - w0 + 3) >> 2 : kMtWinQuads;      // quads of this window
                const bool has_next = w0 + 4 * nq < L;                                     // the boundary sample exists
                const int ns = nq + (has_next ? 1 : 0);
                int nslow = 0;
                // ---- round 1: the first position of every quad, and of the next window's first
                {
                    uint32_t ent[kMtNsp];                         // bases left (capped at 65535) << 16 | position - w0
                    MtProbe pr[kMtNsp];
#pragma unroll
                    for (int s = 0; s < kMtNsp; s++) {
                        const int t0 = 64 * s + lane;
                        const int t = t0 < ns ? t0 : 0;
                        const int a = w0 + 4 * t;
                        const int m = t0 < ns ? L - a : 0;
                        ent[s] = (uint32_t)m << 16 | (uint32_t)(4 * t);
                        const uint32_t o = 2u * (uint32_t)a + 1u;
                        const uint32_t *dq = Dp + (o >> 5);
                        const uint32_t sh = 32u - (o & 31u);
                        const uint32_t d0 = dq[0], d1 = dq[1], d2 = dq[2];
                        pr[s] = mt_issue<C16>(mtab, __builtin_amdgcn_alignbit(d0, d1, sh), __builtin_amdgcn_alignbit(d1, d2, sh), P2);
                    }
                    mt_v4i rb[kMtNsp];
#pragma unroll
                    for (int s = 0; s < kMtNsp; s++) rb[s] = mt_second<C16>(mtab, pr[s]);
#pragma unroll
                    for (int s = 0; s < kMtNsp; s++) {
                        bool slow;
                        const int best0 = mt_eval<C16>(pr[s], rb[s], P2, slow);
                        const int rel = (int)(ent[s] & 0xFFFFu), m = (int)(ent[s] >> 16);
                        const int best = best0 < m ? best0 : m;
                        if (m) fwW[rel] = (uint16_t)(w0 + rel + best);
                        slow = slow && m > best0;
                        const unsigned long long sb = __ballot(slow);
                        if (slow) sl[nslow + __popcll(sb & ((1ull << lane) - 1ull))] = (uint16_t)rel;
                        nslow += __popcll(sb);
                    }
                }
                wave_lds_fence();
#pragma nounroll
                for (int c0 = 0; c0 < nslow; c0 += kWave)
                    mt_slow<true, C16>(ix, mtab, ov, mode, lane, c0, nslow, sl, Dp, DW, nullptr, nullptr, 0, L, w0, fwW);
                wave_lds_fence();
                // ---- round 2: the other three positions of a quad where its sample and the next quad's differ
                nslow = 0;
#pragma nounroll
                for (int t0 = lane; t0 < nq + lane; t0 += kWave) {
                    const int t = t0 < nq ? t0 : 0;
                    const int rel = 4 * t, a = w0 + rel;
                    const int m = t0 < nq ? L - a : 0;                                    // > 0 for every quad of the window
                    const uint32_t v0 = fwW[rel];
                    uint32_t v1 = v0, v2 = v0, v3 = v0;
                    const bool has_right = m > 4;
                    const uint32_t v4 = has_right ? fwW[rel + 4] : 0u;
                    const bool need = m > 1 && ((flags & 1) || ((int)v0 != L && !(has_right && v4 == v0)));
                    bool s1 = false, s2 = false, s3 = false;
                    if (need) {
                        const uint32_t o = 2u * (uint32_t)a + 1u;
                        const uint32_t *dq = Dp + (o >> 5);
                        const MtQuad q = mt_quad_interior<C16>(mtab, P2, dq[0], dq[1], dq[2], 32u - (o & 31u), a, m, L, v0, has_right, v4,
                                                               (flags & 1) != 0);
                        s1 = q.s1;
                        s2 = q.s2;
                        s3 = q.s3;
                        v1 = q.v1;
                        v2 = q.v2;
                        v3 = q.v3;
                    }
                    if (m) *reinterpret_cast<uint2 *>(fwW + rel) = make_uint2(v0 | v1 << 16, v2 | v3 << 16);
                    const unsigned long long sb1 = __ballot(s1), sb2 = __ballot(s2), sb3 = __ballot(s3);
                    if (sb1 | sb2 | sb3) {
                        const unsigned long long below = (1ull << lane) - 1ull;
                        const int n1 = __popcll(sb1), n2 = __popcll(sb2);
                        if (s1) sl[nslow + __popcll(sb1 & below)] = (uint16_t)(rel + 1);
                        if (s2) sl[nslow + n1 + __popcll(sb2 & below)] = (uint16_t)(rel + 2);
                        if (s3) sl[nslow + n1 + n2 + __popcll(sb3 & below)] = (uint16_t)(rel + 3);
                        nslow += n1 + n2 + __popcll(sb3);
                    }
                }
                wave_lds_fence();
#pragma nounroll
                for (int c0 = 0; c0 < nslow; c0 += kWave)
                    mt_slow<true, C16>(ix, mtab, ov, mode, lane, c0, nslow, sl, Dp, DW, nullptr, nullptr, 0, L, w0, fwW);
                wave_lds_fence();
                // ---- this window's results: fwd values (two per dword)
                const int npos = L - w0 < kMtWinPos ? L - w0 : kMtWinPos;
                {
                    uint32_t *dst = reinterpret_cast<uint32_t *>(frow + w0);             // w0 is even: dword aligned
                    const uint32_t *src = reinterpret_cast<const uint32_t *>(fwW);
                    for (int i = lane; i < (npos + 1) >> 1; i += kWave) dst[i] = src[i];
                }
                wave_lds_fence();
            }
        }
        wave_lds_fence();
        r = r_next;
    }
}

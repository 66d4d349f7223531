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
constexpr int kMtTarget = 768;     // ... so that a group holds about this many positions (one pass of 3 x 64 quads) ...
constexpr int kMtTarget2 = 1536;   // ... or two full passes, where the larger group costs no resident block (plan_find_smems)
constexpr int kMtSlowCap = 512;    // entries of the slow list where a group has more positions than that (at least kMtNsp x 64)


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
// entries of the slow list: one per position of the group -- no list can get longer -- up to kMtSlowCap; a group with more
// positions than that runs its slow passes whenever the next lookup pass could overflow the list (match_table_body.inc)
__host__ __device__ inline int mt_slow_cap(int grp, int max_len) { return grp * max_len <= kMtSlowCap ? grp * max_len : kMtSlowCap; }
__host__ __device__ inline int mt_wave_bytes(int grp, int max_len, int qp_recs, int fwd_stride)
{
    return mt_r16(grp * mt_short_row_dwords(max_len, qp_recs) * 4) + 64 + mt_r16(grp * fwd_stride) + mt_r16(mt_slow_cap(grp, max_len) * 2) +
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
// RC (genie_find_smems_both, match_table_both_kernel): N counts strand-reads, two per input row; strand-read v is row v >> 1 as
// given (v even) or its reverse complement (v odd), built while packing.  `vlens` (RC with lens only) gets every strand-read's
// length for K_B.  Both kernels share one body, match_table_body.inc.
template <int WPS, bool C16, bool PK>
__global__ void __launch_bounds__(512, WPS) match_table_kernel(DevIndex ix, int mode, const uint8_t *__restrict__ reads,
                                                             const int32_t *__restrict__ lens, long long N, int stride,
                                                             int fixed_len, uint8_t *__restrict__ fwd_out, int fwd_stride,
                                                             RefRec *__restrict__ qp_out, int qp_recs, int qp_stride,
                                                             int32_t *__restrict__ status, int grp, int max_len,
                                                             long long mtab_bytes, int flags, int cus)
{
    constexpr bool RC = false;
    int32_t *const vlens = nullptr;
#include "match_table_body.inc"
}
// both strands: N = 2 x the input rows
template <int WPS, bool C16>
__global__ void __launch_bounds__(512, WPS) match_table_both_kernel(DevIndex ix, int mode, const uint8_t *__restrict__ reads,
                                                                  const int32_t *__restrict__ lens, long long N, int stride,
                                                                  int fixed_len, uint8_t *__restrict__ fwd_out, int fwd_stride,
                                                                  RefRec *__restrict__ qp_out, int qp_recs, int qp_stride,
                                                                  int32_t *__restrict__ status, int grp, int max_len,
                                                                  long long mtab_bytes, int flags, int cus, int32_t *__restrict__ vlens)
{
    constexpr bool PK = false, RC = true;
#include "match_table_body.inc"
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

// RC (match_table_long_both_kernel): as in match_table_both_kernel, N strand-reads, two per input row, the odd ones
// reverse-complemented while packing.  Both kernels share one body, match_table_long_body.inc.
template <bool C16>
__global__ void __launch_bounds__(512, 8) match_table_long_kernel(DevIndex ix, int mode, const uint8_t *__restrict__ reads,
                                                                  const int32_t *__restrict__ lens, long long N, int stride,
                                                                  int fixed_len, uint8_t *__restrict__ fwd_out, int fwd_stride,
                                                                  RefRec *__restrict__ qp_out, int qp_recs,
                                                                  int32_t *__restrict__ status, int max_len, long long mtab_bytes,
                                                                  int flags, int cus)
{
    constexpr bool RC = false;
    int32_t *const vlens = nullptr;
#include "match_table_long_body.inc"
}
// both strands: N = 2 x the input rows
template <bool C16>
__global__ void __launch_bounds__(512, 8) match_table_long_both_kernel(DevIndex ix, int mode, const uint8_t *__restrict__ reads,
                                                                       const int32_t *__restrict__ lens, long long N, int stride,
                                                                       int fixed_len, uint8_t *__restrict__ fwd_out, int fwd_stride,
                                                                       RefRec *__restrict__ qp_out, int qp_recs,
                                                                       int32_t *__restrict__ status, int max_len, long long mtab_bytes,
                                                                       int flags, int cus, int32_t *__restrict__ vlens)
{
    constexpr bool RC = true;
#include "match_table_long_body.inc"
}

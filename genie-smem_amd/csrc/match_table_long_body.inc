// match_table_long_body.inc -- the body of K_A for reads of 256 .. 8192 bases (match_table_kernel.inc), included as the body
// of match_table_long_kernel and of match_table_long_both_kernel, which declare RC and `vlens` before the include (as
// match_table_body.inc).
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
    const long long share0 = (N + gridDim.x - 1) / gridDim.x;
    const long long share = RC ? (share0 + 1) & ~1ll : share0;          // both strands of a read in one block
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
        const long long row = RC ? r >> 1 : r;
        const bool rev = RC && (r & 1);
        if (touch_ahead && stride > 0 && stride <= 4096 && r_next < r_stop && (!RC || (r_next >> 1) != row))
            scalar_touch_lines(reads + (RC ? r_next >> 1 : r_next) * (long long)stride, (uint32_t)stride);
        int L = lens ? lens[row] : fixed_len;
        if (RC && lens && lane == 0) vlens[r] = L;
        int st = GENIE_READ_OK;
        if (L < 0 || L > max_len) { st = GENIE_READ_BAD_BASE; L = 0; }         // host validates lengths; defensive only
        // ---- pack: 64 dwords (1024 bases) per pass; every dword of the row is rewritten (zeros behind the read)
        {
            const uint8_t *base = reads + row * (long long)stride;
            bool bad = false;
            uint32_t carry = 0;                                                // the dword before this pass's first
            for (int j0 = 0; j0 < DW; j0 += kWave) {
                const int j = j0 + lane;
                const int left = L - 16 * j;
                uint32_t v[4] = {0, 0, 0, 0};
                if (rev) {
                    // the reverse strand: dword k of piece j = the bytes F[L-16j-4k-4 .. L-16j-4k) in reverse order; the last,
                    // partial piece byte by byte from the row (its window would start before the row)
                    if (left >= 16) {
#pragma unroll
                        for (int k = 0; k < 4; k++) v[k] = __builtin_bswap32(*reinterpret_cast<const u32_unaligned *>(base + L - 16 * j - 4 * k - 4));
                    } else if (left > 0) {
                        for (int b = 0; b < left; b++) v[b >> 2] |= (uint32_t)base[left - 1 - b] << (8 * (b & 3));
                    }
                } else if (left >= 16) {
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
                uint32_t d = (mt_pack4(v[0]) << 24) | (mt_pack4(v[1]) << 16) | (mt_pack4(v[2]) << 8) | mt_pack4(v[3]);
                if (rev && left > 0) d ^= left >= 16 ? ~0u : ~0u << (32 - 2 * left);          // complement: code c -> 3 - c
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

// match_table_body.inc -- the body of K_A for reads of up to 255 bases (match_table_kernel.inc), included as the body of
// match_table_kernel and of match_table_both_kernel.  Each kernel declares RC (both strands) and PK (2-bit packed reads) as
// compile-time constants and `vlens` before the include.  (A __device__ function that both kernels call would be optimized
// on its own before it is inlined, and the existing kernels' code would change with it; the text is shared instead.)
    static_assert(!(PK && RC), "both strands of 2-bit packed reads are not built");
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
    uint16_t *qa = reinterpret_cast<uint16_t *>(reinterpret_cast<uint8_t *>(sl) + mt_r16(mt_slow_cap(grp, max_len) * 2));
    uint16_t *qb = qa + grp * mt_quads(max_len);
    for (int i = lane; i < grp * DW; i += kWave) Dp[i] = 0;                    // the zero padding behind every read
    // The slow list holds mt_slow_cap entries.  Where that is fewer than the group has positions, a lookup pass runs only while
    // the list has room for all it can add (kMtNsp x 64 entries in round 1, 64 in round 2); otherwise the pending slow passes
    // run first and empty the list.  That changes no result: a slow item writes its own byte of fwL only, over the provisional
    // value its lookup pass wrote before; round 2 starts after all of round 1's slow items, and a slow middle puts both its
    // neighbours on qb whatever it resolves to.  An uncapped list never fills (nslow <= positions = its capacity).
    const uint8_t *reads_end = reads + (RC ? N >> 1 : N) * (long long)stride;

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
            if (RC) scalar_touch_lines(reads + (rn >> 1) * (long long)stride, (uint32_t)((((rn + rows - 1) >> 1) - (rn >> 1) + 1) * stride));
            else scalar_touch_lines(reads + rn * (long long)stride, (uint32_t)(rows * stride));
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
                const long long row = RC ? (r + u) >> 1 : r + u;
                const bool rev = RC && ((r + u) & 1);
                L = lens ? lens[row] : fixed_len;
                if (RC && lens && pj == 0) vlens[r + u] = L;
                if (L < 0 || L > max_len) { st = GENIE_READ_BAD_BASE; L = 0; }       // host validates lengths; defensive only
                const int left = L - 16 * pj;
                if (PK) {
                    if (left > 0) {
                        d = __builtin_bswap32(*reinterpret_cast<const uint32_t *>(reads + (r + u) * (long long)stride + 4 * pj));
                        if (left < 16) d &= ~0u << (32 - 2 * left);                 // whatever lies behind the read is not part of it
                    }
                }
                const uint8_t *src = reads + row * (long long)stride + 16 * pj;
                uint32_t v[4] = {0, 0, 0, 0};
                if (PK) {
                } else if (rev) {
                    // dword pj of the reverse strand: the 16 bytes F[L-16-16pj .. L-16pj) of the row F, in reverse order (and
                    // complemented below, after the bad-base test).  The last piece's window starts before the row; it is
                    // loaded whole where it still lies inside the input, byte by byte from the row where it would not.
                    const long long o = row * (long long)stride + L - 16 - 16 * pj;
                    if (left >= 16 || (left > 0 && o >= 0)) {
                        const nt_u4 q = *reinterpret_cast<const nt_u4_unaligned *>(reads + o);
                        v[0] = __builtin_bswap32(q.w); v[1] = __builtin_bswap32(q.z); v[2] = __builtin_bswap32(q.y); v[3] = __builtin_bswap32(q.x);
                        if (left < 16) {
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                const int nb = left - 4 * k;                      // bytes of dword k that belong to the read
                                v[k] = nb >= 4 ? v[k] : (nb <= 0 ? 0u : v[k] & ((1u << (8 * nb)) - 1u));
                            }
                        }
                    } else if (left > 0) {
                        const uint8_t *f = reads + row * (long long)stride;
                        for (int b = 0; b < left; b++) v[b >> 2] |= (uint32_t)f[left - 1 - b] << (8 * (b & 3));
                    }
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
                    if (rev && left > 0) d ^= left >= 16 ? ~0u : ~0u << (32 - 2 * left);      // complement: code c -> 3 - c
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
            // a 64-entry pass fits the list while nslow <= flush_at; worked out per group (the empty asm keeps it from being hoisted)
            // so that it is not one more scalar kept across the pack stage: the kernel is at its scalar-register limit
            int positions = grp * max_len;
            asm volatile("" : "+s"(positions));
            const int flush_at = positions > kMtSlowCap ? kMtSlowCap - kWave : 1 << 30;
            const int n1 = (dbg & 4) ? 0 : nquads;
            int c0 = 0;
            do {
#pragma nounroll
            for (; c0 < n1 && nslow + (kMtNsp - 1) * kWave <= flush_at; c0 += kMtNsp * kWave) {
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
            for (int s0 = 0; s0 < ((dbg & 1) ? 0 : nslow); s0 += kWave) mt_slow<false, C16>(ix, mtab, ov, mode, lane, s0, nslow, sl, Dp, DW, Ls, fwL, FS);
            wave_lds_fence();
            nslow = 0;
            } while (__builtin_expect(c0 < n1, 0));                                    // more than once only where the list filled up
            // ---- round 2: the other three positions of a quad, looked up only where the quad's sample and the next
            // quad's differ (and the match does not already reach the end of the read): the MIDDLE position first, a
            // neighbour only where the middle leaves it open (fwd[] is non-decreasing: fwd[a+2] == fwd[a] settles a+1,
            // fwd[a+2] == fwd[a+4] or == L settles a+3).  Three passes, each over a DENSE list, so that every lane of a
            // lookup pass has work (a lane per quad with two dependent lookups inside ran at a third of the lanes and
            // three times the instructions per lookup of round 1): the quads to work on, their middles, the neighbours.
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
            int cm = 0, cn = 0;                                   // middles and neighbours looked up so far
            do {
#pragma nounroll
            for (; cm < nqa && nslow <= flush_at; cm += kWave) {
                const bool valid = cm + lane < nqa;
                const uint32_t it = qa[valid ? cm + lane : 0];
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
            // the neighbours (positions a + 1 and a + 3) that the middles left open, once all the middles are done
#pragma nounroll
            for (; cm >= nqa && cn < nqb && nslow <= flush_at; cn += kWave) {
                const bool valid = cn + lane < nqb;
                const uint32_t it = qb[valid ? cn + lane : 0];
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
            for (int s0 = 0; s0 < ((dbg & 1) ? 0 : nslow); s0 += kWave) mt_slow<false, C16>(ix, mtab, ov, mode, lane, s0, nslow, sl, Dp, DW, Ls, fwL, FS);
            wave_lds_fence();
            nslow = 0;
            } while (__builtin_expect(cm < nqa || cn < nqb, 0));                       // more than once only where the list filled up
            // ---- results: fwd rows
            const int nrows = N - r < (long long)grp ? (int)(N - r) : grp;
            uint4 *dst = reinterpret_cast<uint4 *>(fwd_out + r * (long long)FS);                  // rows are multiples of 16 bytes
            const uint4 *src = reinterpret_cast<const uint4 *>(fwL);
            for (int i = lane; i < ((dbg & 32) ? 0 : nrows * (FS >> 4)); i += kWave) store_nt(dst + i, src[i]);
        }
        wave_lds_fence();
        gi = gi_next;
    }

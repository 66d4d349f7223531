// lu_seg_body.inc -- the body of LU1 / LU2 (long_units.inc), included once per kernel with LU_SEG_USABLE set to the mask of
// usable bases (bit b for base b): the kernels differ in that expression alone, and lu_seg_kernel stays the code it was.
    __shared__ uint8_t sflag[kLuSub + 8];
    __shared__ int wtot[4];
    const int t = threadIdx.x, lane = t & (kWave - 1), wave = t >> 6;
    const long long c0 = (long long)blockIdx.x * kLuChunk;
    long long run = 0;                                           // starts in front of the current kLuSub positions
    if (SCATTER) {
        const long long a = (long long)bsum[blockIdx.x], b = (long long)bsum[blockIdx.x + 1];
        if (b <= p0 || a > p1) return;                           // block-uniform: no unit of the pass begins or ends here
        run = a;
    }
    const uint32_t present = LU_SEG_USABLE;
    const long long vlo = R.at(0), vhi = R.at(R.count());
    long long q0 = R.find(c0);
    LuSr s0 = lu_sr(R, q0), s1 = lu_sr(R, q0 + 1 < R.count() ? q0 + 1 : q0);
    bool brk = false;
    for (int sub = 0; sub < kLuChunk / kLuSub; sub++) {
        const long long cs = c0 + sub * kLuSub;
        if (cs >= vhi) break;                                    // block-uniform
        if (cs >= s0.at + (s0.o2 - s0.o)) {
            q0 = R.find(cs);
            s0 = lu_sr(R, q0);
            s1 = lu_sr(R, q0 + 1 < R.count() ? q0 + 1 : q0);
        }
        const long long len0 = s0.o2 - s0.o, pb = cs - 1 - s0.at;
        if (pb >= 0 && pb + kLuSub + 2 <= len0) {                // all inside one strand-read (block-uniform): 32-bit work only
            const uint8_t *b0 = R.bases + (s0.rev ? s0.o2 - 1 - pb : s0.o + pb);
            const int jf = pb == 0 ? 0 : -1, jl = len0 - 1 - pb <= kLuSub + 1 ? (int)(len0 - 1 - pb) : -1;
            const uint32_t x = s0.rev ? 3u : 0u;
            for (int j = t; j < kLuSub + 2; j += 256) {
                const uint32_t c = s0.rev ? b0[-j] : b0[j];
                const bool good = c < 4u && ((present >> (c ^ x)) & 1u);
                sflag[j] = (uint8_t)((good ? 1u : 0u) | (j == jf ? 2u : 0u) | (j == jl ? 4u : 0u) | 8u);
            }
        } else {
            for (int j = t; j < kLuSub + 2; j += 256) sflag[j] = (uint8_t)lu_flags(R, present, cs - 1 + j, vlo, vhi, s0, s1);
        }
        __syncthreads();
        uint32_t f[kLuPer + 2];
#pragma unroll
        for (int i = 0; i < kLuPer + 2; i++) f[i] = sflag[kLuPer * t + i];
        uint32_t sm = 0, em = 0;
#pragma unroll
        for (int i = 0; i < kLuPer; i++) {
            const uint32_t cur = f[i + 1];
            const bool g = cur & 1u;
            if (g && ((cur & 2u) || !(f[i] & 1u))) sm |= 1u << i;
            if (g && ((cur & 4u) || !(f[i + 2] & 1u))) em |= 1u << i;
            brk = brk || (cur & 9u) == 8u;
        }
        const int cnt = __popc(sm);
        int inc = cnt;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int x = __shfl_up(inc, o, kWave);
            if (lane >= o) inc += x;
        }
        if (lane == kWave - 1) wtot[wave] = inc;
        __syncthreads();
        int all = 0;
        long long seen = run + inc - cnt;                        // starts in front of the thread's positions
        for (int w = 0; w < 4; w++) {
            const int x = wtot[w];
            seen += w < wave ? x : 0;
            all += x;
        }
        const long long v0 = cs + kLuPer * t;
        if (!SCATTER) {
#pragma unroll
            for (int i = 0; i < kLuPer; i++) {
                if (f[i + 1] & 2u) {                             // a strand-read begins: also the empty ones that sit here
                    const long long v = v0 + i;
                    const int32_t loc = (int32_t)(seen + __popc(sm & ((1u << i) - 1u)));
                    const long long q = R.find(v);
                    qloc[q] = loc;
                    for (long long e = q - 1; e >= 0 && R.at(e) == v; e--) qloc[e] = loc;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < kLuPer; i++) {
                if ((sm >> i) & 1u) seen++;
                const long long k = seen - 1;                    // the segment a good position belongs to
                if (k >= p0 && k < p1) {
                    if ((sm >> i) & 1u) ua[k - p0] = v0 + i;
                    if ((em >> i) & 1u) ub[k - p0] = v0 + i + 1;
                }
            }
        }
        run += all;
        __syncthreads();
    }
    if (!SCATTER) {
        // one writer per block, and none once the flag is up
        if (__syncthreads_or(brk) && t == 0 && __hip_atomic_load(anybreak, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
            atomicOr(anybreak, 1);
        if (t == 0) bsum[blockIdx.x] = (unsigned long long)run;
    }

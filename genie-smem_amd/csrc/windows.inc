// windows.inc -- genie_rescue_windows and genie_window_mems: where to look for a mate next to its partner, and the MEMs of a
// strand-read against such a window of the reference, merged into the MEM rows of the batch (included by kernels.hip behind
// align.inc, which ends with pairs.inc, inside namespace genie).  The definitions are the header's; DESIGN.md section 27 has
// the reasoning.
//
// genie_rescue_windows
//   RW0 chain_check_kernel   the record offsets; the host reads the flag: the call's one synchronisation
//   RW1 rescue_plan_kernel   one lane per read: is it a target, and the windows of its two units
//   RW2 rescue_totals_kernel the three totals, by one block
// genie_window_mems.  No index is consulted: a window is compared with the strand-read base for base, 32 bases a step.
//   WM0 lu_check_kernel, chain_check_kernel   the read offsets and the input row offsets; one flag, one synchronisation
//   WM1 window_mark_kernel   one lane per unit: its window clamped, its input rows counted, 1 for a unit to search
//   WM2 launch_compact       the units to search as a list
//   WM3 window_wave_kernel<false>  one wave per listed unit, grid-stride over the list.  The strand-read is packed to 2 bits a
//                            base in LDS (and, only where it has one, the mask of its codes > 3); the unit's input rows go to
//                            the front of a table of GENIE_WINDOW_MAX_ROWS rows in LDS.  Lane l takes the diagonals d = t - p
//                            l, l + 64, ... of the rectangle read x window and walks each in 32-base words: the XOR of the
//                            query word with the reference word, folded to one bit a base; a maximal run of zeros of at least
//                            min_len bases is a row and goes behind the input rows.  Words of too many mismatches to hold such
//                            a run cost two bit scans (the run that ends and the run that begins there) and no loop.  Then the
//                            rows that repeat an earlier row's (start, end, pos) are counted: what is left is the unit's count.
//   WM4 launch_compact       the counts scanned into d_offsets
//   WM5 window_wave_kernel<true>   the same walk; the repeats are squeezed out of the table and every row goes to the place
//                            that the number of smaller keys gives it: a counting rank over at most 2048 keys in LDS
//   WM6 window_copy_kernel   one lane per input row: the rows of the units that were not merged, as they are
//   WM7 window_totals_kernel the three totals, by one block
// The slot of a found row in the LDS table comes from one integer atomicAdd in LDS.  It decides no value: the rows found are
// distinct, all of them sit behind the input rows, and the output order is the rank of the keys.
namespace {

constexpr int kWinMax = GENIE_WINDOW_MAX;                     // bases of a window
constexpr int kWinRows = GENIE_WINDOW_MAX_ROWS;               // rows of a searched unit, input rows included
constexpr int kWinQWords = GENIE_MAX_READ_LEN / 32 + 8;       // 64-bit words of the packed strand-read: one spare word is read
constexpr int kWinSearched = 1, kWinRowCap = 2, kWinTooLong = 4;
static_assert(4 * (kWinRows * 16 + 2 * kWinQWords * 8 + 16) <= 160 * 1024, "four waves per CU");

// ------------------------------------------------------------------ genie_rescue_windows
struct RescueArea {
    int *flag;                            // RW0's verdict
    int32_t *target;                      // per read: 1 for a target
};

inline int64_t rescue_layout(uint8_t *base, int64_t N, RescueArea *a)
{
    Carver c{base};
    c.take(a->flag, 8);
    c.take(a->target, N * 4);
    return c.at;
}

struct RescueInput {
    const long long *ctg;                 // or null: one contig [0, n)
    long long nctg;
    const long long *roff, *so;
    long long N;
    const int4 *rec;
    long long n_records;
    const int4 *pairs;
    int orient, isize_max, min_anchor;
};

// [lo, hi) inside a contig of clen bases that starts at clo -> the window in the concatenation, (0, 0) for none
__device__ __forceinline__ int2 rescue_cut(long long lo, long long hi, long long clo, long long clen)
{
    lo = sel_clamp(lo, 0, clen);
    hi = sel_clamp(hi, 0, clen);
    if (hi <= lo) return make_int2(0, 0);
    if (hi - lo > kWinMax) hi = lo + kWinMax;
    return make_int2((int)(clo + lo), (int)(clo + hi));
}

__global__ void __launch_bounds__(256) rescue_plan_kernel(DevIndex ix, RescueInput in, int2 *__restrict__ windows, int32_t *__restrict__ target)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= in.N) return;
    int2 w[2] = {make_int2(0, 0), make_int2(0, 0)};
    int tgt = 0;
    const long long R = sel_clamp(in.so[in.N], 0, in.n_records);
    const int4 pr = in.pairs[2 * (r >> 1)];
    const long long a = (r & 1) ? pr.x : pr.y;                       // the chosen record of the other mate
    if ((pr.z & 1) == 0 && a >= 0 && a < R && in.rec[3 * a + 2].y >= in.min_anchor) {
        tgt = 1;
        if (in.roff[r + 1] > in.roff[r]) {                           // a read without bases has nothing to seed
            const int4 r1 = in.rec[3 * a + 1];
            const int sa = in.rec[3 * a].w != 0 ? 1 : 0;
            long long clo = 0, chi = ix.n;
            if (in.ctg) {
                const long long c = sel_clamp(r1.x, 0, in.nctg - 1);
                clo = sel_clamp(in.ctg[c], 0, ix.n);
                chi = sel_clamp(in.ctg[c + 1], clo, ix.n);
            }
            const long long b = (long long)r1.y - 1, e = b + r1.z, most = in.isize_max;
            const bool fr = (in.orient & 1) != 0, rf = (in.orient & 2) != 0;
            const bool right = (fr && sa == 0) || (rf && sa == 1), left = (fr && sa == 1) || (rf && sa == 0);
            if (right || left) w[1 - sa] = rescue_cut(left ? e - most : b, right ? b + most : e, clo, chi - clo);
            if (in.orient & 4) w[sa] = rescue_cut(e - most, b + most, clo, chi - clo);
        }
    }
    windows[2 * r] = w[0];
    windows[2 * r + 1] = w[1];
    if (target) target[r] = tgt;
}

// {units with a window, pairs with at least one, reads that are targets}, by one block
__global__ void __launch_bounds__(kScanBlock) rescue_totals_kernel(const int2 *__restrict__ windows, const int32_t *__restrict__ target,
                                                                   long long P, long long *__restrict__ totals)
{
    __shared__ unsigned long long wsum[3][kScanBlock / kWave];
    unsigned long long a = 0, b = 0, c = 0;
    for (long long k = threadIdx.x; k < P; k += kScanBlock) {
        unsigned n = 0;
        for (int j = 0; j < 4; j++) {
            const int2 w = windows[4 * k + j];
            n += w.y > w.x ? 1u : 0u;
        }
        a += n;
        b += n ? 1u : 0u;
        c += (unsigned)(target[2 * k] + target[2 * k + 1]);
    }
    a = wave_sum64(a);
    b = wave_sum64(b);
    c = wave_sum64(c);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        wsum[0][threadIdx.x / kWave] = a;
        wsum[1][threadIdx.x / kWave] = b;
        wsum[2][threadIdx.x / kWave] = c;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long all = 0;
        for (int w = 0; w < kScanBlock / kWave; w++) all += wsum[threadIdx.x][w];
        totals[threadIdx.x] = (long long)all;
    }
}

// ------------------------------------------------------------------ genie_window_mems
struct WinArea {
    int *flag;                            // WM0's verdict
    int2 *win;                            // per unit: its window, clamped
    int32_t *has, *cnt, *added, *st;      // per unit: 1 to search; output rows; window rows that are new; status
    int4 *slot, *list;                    // per unit: its index as a row, and the rows of the units to search
    long long *loff;                      // U + 1
    uint8_t *scan_tmp;                    // launch_compact's
};

inline int64_t win_layout(uint8_t *base, int64_t U, WinArea *a)
{
    Carver c{base};
    c.take(a->flag, 8);
    c.take(a->win, U * 8);
    c.take(a->has, U * 4);
    c.take(a->cnt, U * 4);
    c.take(a->added, U * 4);
    c.take(a->st, U * 4);
    c.take(a->slot, U * 16);
    c.take(a->list, U * 16);
    c.take(a->loff, (U + 1) * 8);
    c.take(a->scan_tmp, compact_tmp_bytes(U));
    return c.at;
}

struct WinInput {
    const long long *in_off;              // or null: no input rows
    const int4 *in_rows;
    long long U;
    int m;
};

// WM1
__global__ void __launch_bounds__(256) window_mark_kernel(DevIndex ix, LuReads R, WinInput in, const int2 *__restrict__ windows,
                                                          int2 *__restrict__ win, int32_t *__restrict__ has, int4 *__restrict__ slot,
                                                          int32_t *__restrict__ cnt, int32_t *__restrict__ added, int32_t *__restrict__ st,
                                                          int32_t *__restrict__ status)
{
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= in.U) return;
    const int2 w = windows[u];
    const int wb = (int)sel_clamp(w.x, 0, ix.n);
    int we = (int)sel_clamp(w.y, 0, ix.n);
    we = we < wb ? wb : we;
    we = we - wb > kWinMax ? wb + kWinMax : we;
    const LuSr sr = lu_sr(R, u);
    const bool search = we > wb && sr.o2 - sr.o <= GENIE_MAX_READ_LEN;
    const int s = we > wb && !search ? kWinTooLong : 0;
    win[u] = make_int2(wb, we);
    has[u] = search ? 1 : 0;
    slot[u] = make_int4((int)u, 0, 0, 0);
    cnt[u] = in.in_off ? (int)(in.in_off[u + 1] - in.in_off[u]) : 0;
    added[u] = 0;
    st[u] = s;                                                       // WM3 overwrites it for a listed unit
    if (status) status[u] = s;
}

// (start, pos, end) of row b below that of row a
__device__ __forceinline__ bool win_key_less(const int4 &b, const int4 &a)
{
    return b.x < a.x || (b.x == a.x && (b.z < a.z || (b.z == a.z && b.y < a.y)));
}

// WM3 (FILL false) / WM5
template <bool FILL>
__global__ void __launch_bounds__(kWave) window_wave_kernel(DevIndex ix, LuReads R, WinInput in, const long long *__restrict__ loff,
                                                            const int4 *__restrict__ list, const int2 *__restrict__ win,
                                                            int32_t *__restrict__ cnt, int32_t *__restrict__ added, int32_t *__restrict__ st,
                                                            int32_t *__restrict__ status, const long long *__restrict__ out_off,
                                                            int4 *__restrict__ out, long long cap)
{
    __shared__ int4 rows[kWinRows];
    __shared__ uint64_t qb[kWinQWords], qv[kWinQWords];
    __shared__ int nfound;
    const int lane = threadIdx.x;
    const long long nl = sel_clamp(loff[in.U], 0, in.U);
    for (long long k = blockIdx.x; k < nl; k += gridDim.x) {
        const long long u = sel_clamp(list[k].x, 0, in.U - 1);
        if (FILL && st[u] != kWinSearched) continue;
        const int2 w = win[u];
        const LuSr sr = lu_sr(R, u);
        const int L = (int)(sr.o2 - sr.o), wb = w.x, we = w.y;
        if (L < 0 || L > GENIE_MAX_READ_LEN || we <= wb) continue;   // not what WM1 listed
        const long long in0 = in.in_off ? in.in_off[u] : 0, nin64 = in.in_off ? in.in_off[u + 1] - in0 : 0;
        wave_lds_fence();                                            // the unit before has read the tables
        if (lane == 0) nfound = 0;
        int found = 0;
        const bool full = nin64 > kWinRows;
        const int nin = full ? 0 : (int)nin64;
        if (!full) {
            for (int j = lane; j < nin; j += kWave) rows[j] = in.in_rows[in0 + j];
            // the strand-read, four bases a byte; base j of a word in bits [62 - 2j, 63 - 2j] as in the packed reference
            const int bytes = (((L + 31) >> 5) + 1) * 8;
            bool bad = false;
            for (int g = lane; g < bytes; g += kWave) {
                unsigned q = 0, v = 0;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int p = 4 * g + e;
                    unsigned c = 0, inv = 0;
                    if (p < L) {
                        c = R.bases[sr.rev ? sr.o2 - 1 - p : sr.o + p];
                        inv = c > 3u ? 1u : 0u;
                        c = inv ? 0u : (sr.rev ? c ^ 3u : c);
                    }
                    q = (q << 2) | c;
                    v = (v << 2) | inv;
                }
                const int at = (g & ~7) | (7 - (g & 7));
                reinterpret_cast<uint8_t *>(qb)[at] = (uint8_t)q;
                reinterpret_cast<uint8_t *>(qv)[at] = (uint8_t)v;
                bad = bad || v != 0;
            }
            const bool any_bad = __ballot(bad) != 0ull;
            wave_lds_fence();
            const int D = L > 0 ? L + (we - wb) - 1 : 0, dmin = wb - (L - 1);
            for (int k0 = 0; k0 < D; k0 += kWave) {
                const int d = dmin + k0 + lane;
                const int p_lo = wb - d > 0 ? wb - d : 0, p_hi = k0 + lane < D ? (we - d < L ? we - d : L) : 0;
                int run = p_lo;                                      // where the open run of matches began
                auto emit = [&](int a, int b) {
                    if (b - a < in.m) return;
                    const int at = nin + atomicAdd(&nfound, 1);
                    if (at < kWinRows) rows[at] = make_int4(a, b, d + a + 1, -1);
                };
                for (int p = p_lo; p < p_hi; p += 32) {
                    const uint64_t x = qwin(qb, p) ^ rwin(ix.ref, d + p);
                    uint64_t mm = x | (x >> 1);
                    if (any_bad) mm |= qwin(qv, p);
                    mm &= 0x5555555555555555ull;
                    if (p_hi - p < 32) mm |= 0x5555555555555555ull >> (2 * (p_hi - p));
                    if (!mm) continue;
                    int prev = __clzll((long long)mm) >> 1;          // the first base that differs ends the open run
                    emit(run, p + prev);
                    int last = 31 - ((__ffsll((long long)mm) - 1) >> 1);
                    if (prev != last && __popcll(mm) + in.m <= 32) { // few enough mismatches to leave room for a run between two
                        uint64_t rest = mm & ~(1ull << (62 - 2 * prev));
                        while (rest) {
                            const int nx = __clzll((long long)rest) >> 1;
                            rest &= ~(1ull << (62 - 2 * nx));
                            emit(p + prev + 1, p + nx);
                            prev = nx;
                        }
                        last = prev;
                    }
                    run = p + last + 1;
                }
                emit(run, p_hi);
                wave_lds_fence();
                found = *(volatile int *)&nfound;
                if (nin + found > kWinRows) break;
            }
        }
        wave_lds_fence();
        const bool over = full || nin + found > kWinRows;
        if (over) {                                                  // the row cap: the unit keeps its input rows (WM6)
            if (!FILL && lane == 0) {
                st[u] = kWinRowCap;
                if (status) status[u] = kWinRowCap;
            }
            continue;
        }
        // a row that repeats an earlier row's triple: the earlier one is an input row, for the rows found are distinct
        const int K = nin + found;
        unsigned dupmask = 0;
        int ndup = 0, ndup_found = 0;
        for (int c = 0, i = lane; i < K; i += kWave, c++) {
            const int4 a = rows[i];
            const int lim = i < nin ? i : nin;
            bool dup = false;
            for (int j = 0; j < lim; j++) {
                const int4 b = rows[j];
                dup = dup || (b.x == a.x && b.y == a.y && b.z == a.z);
            }
            if (dup) {
                dupmask |= 1u << c;
                ndup++;
                ndup_found += i >= nin ? 1 : 0;
            }
        }
        if (!FILL) {
            ndup = (int)wave_sum64((unsigned long long)ndup);
            ndup_found = (int)wave_sum64((unsigned long long)ndup_found);
            if (lane == 0) {
                cnt[u] = K - ndup;
                added[u] = found - ndup_found;
                st[u] = kWinSearched;
                if (status) status[u] = kWinSearched;
            }
            continue;
        }
        // squeeze the repeats out, in place and in order: a chunk is read whole before it is written, at or in front of itself
        int K2 = 0;
        for (int c = 0, i0 = 0; i0 < K; i0 += kWave, c++) {
            const int i = i0 + lane;
            const bool keep = i < K && ((dupmask >> c) & 1u) == 0;
            const int4 a = keep ? rows[i] : make_int4(0, 0, 0, 0);
            const unsigned long long mask = __ballot(keep);
            wave_lds_fence();
            if (keep) rows[K2 + __popcll(mask & ((1ull << lane) - 1ull))] = a;
            K2 += __popcll(mask);
            wave_lds_fence();
        }
        // the keys are distinct now: a row's place is the number of smaller keys
        const long long off = out_off[u];
        for (int i0 = 0; i0 < K2; i0 += kWave) {
            const int i = i0 + lane;
            const int4 a = rows[i < K2 ? i : 0];
            int less = 0;
            for (int j = 0; j < K2; j++) less += win_key_less(rows[j], a) ? 1 : 0;
            if (i < K2 && off + less < cap) out[off + less] = a;
        }
    }
}

// WM6
__global__ void __launch_bounds__(256) window_copy_kernel(WinInput in, const int32_t *__restrict__ st, const long long *__restrict__ out_off,
                                                          int4 *__restrict__ out, long long cap)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= in.in_off[in.U]) return;
    long long lo = 0, hi = in.U;                                     // the last u in [0, U) with in_off[u] <= j
    while (lo < hi - 1) {
        const long long mid = (lo + hi) >> 1;
        if (in.in_off[mid] <= j) lo = mid; else hi = mid;
    }
    if (st[lo] == kWinSearched) return;                              // WM5 wrote the unit
    const long long at = out_off[lo] + (j - in.in_off[lo]);
    if (at < cap) out[at] = in.in_rows[j];
}

// {rows in all, window rows added after the union, units over a cap}, by one block
__global__ void __launch_bounds__(kScanBlock) window_totals_kernel(const int32_t *__restrict__ added, const int32_t *__restrict__ st,
                                                                   const long long *__restrict__ out_off, long long U,
                                                                   long long *__restrict__ totals)
{
    __shared__ unsigned long long wsum[2][kScanBlock / kWave];
    unsigned long long a = 0, b = 0;
    for (long long u = threadIdx.x; u < U; u += kScanBlock) {
        a += (unsigned)added[u];
        b += (st[u] & (kWinRowCap | kWinTooLong)) ? 1u : 0u;
    }
    a = wave_sum64(a);
    b = wave_sum64(b);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        wsum[0][threadIdx.x / kWave] = a;
        wsum[1][threadIdx.x / kWave] = b;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long all = 0;
        for (int w = 0; w < kScanBlock / kWave; w++) all += wsum[threadIdx.x][w];
        totals[1 + threadIdx.x] = (long long)all;
    }
    if (threadIdx.x == 0) totals[0] = out_off[U];
}

}  // namespace

int64_t rescue_windows_workspace_bytes(int64_t N)
{
    RescueArea a;
    return rescue_layout(nullptr, N, &a);
}

int launch_rescue_windows(const genie_index *ix, const ContigTable &ctg, const RescueBatch &b, int32_t *d_windows, int64_t *d_totals,
                          void *ws, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = b.N;
    if (N == 0) {
        if (d_totals) HIP_TRY(hipMemsetAsync(d_totals, 0, 24, s));
        return GENIE_OK;
    }
    RescueArea a;
    rescue_layout(static_cast<uint8_t *>(ws), N, &a);
    const long long *so = reinterpret_cast<const long long *>(b.sel_offsets);
    HIP_TRY(hipMemsetAsync(a.flag, 0, 8, s));
    LAUNCH_BLOCKS(chain_check_kernel, (N + 1 + 255) / 256, 256, 0, s, so, (long long)N, 0x7fffffffffffffffll, a.flag);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, a.flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return GENIE_E_INVALID;
    const RescueInput in{reinterpret_cast<const long long *>(ctg.offsets), (long long)ctg.n_contigs,
                         reinterpret_cast<const long long *>(b.read_offsets), so, (long long)N, reinterpret_cast<const int4 *>(b.records),
                         (long long)b.n_records, reinterpret_cast<const int4 *>(b.pairs), b.orient, b.isize_max, b.min_anchor_score};
    int2 *windows = reinterpret_cast<int2 *>(d_windows);
    LAUNCH_BLOCKS(rescue_plan_kernel, (N + 255) / 256, 256, 0, s, ix->dev, in, windows, a.target);
    if (d_totals)
        LAUNCH(rescue_totals_kernel, dim3(1), dim3(kScanBlock), 0, s, static_cast<const int2 *>(windows),
               static_cast<const int32_t *>(a.target), (long long)(N / 2), reinterpret_cast<long long *>(d_totals));
    return GENIE_OK;
}

int64_t window_mems_workspace_bytes(int64_t U)
{
    WinArea a;
    return win_layout(nullptr, U, &a);
}

int launch_window_mems(const genie_index *ix, const CsrBatch &b, const WindowBatch &wb, const CsrRows &out, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t U = wb.U;
    if (U == 0) {
        HIP_TRY(hipMemsetAsync(out.offsets, 0, 8, s));
        if (out.totals) HIP_TRY(hipMemsetAsync(out.totals, 0, 24, s));
        return GENIE_OK;
    }
    WinArea a;
    win_layout(static_cast<uint8_t *>(b.ws), U, &a);
    const long long *roff = reinterpret_cast<const long long *>(b.read_offsets);
    const long long *in_off = reinterpret_cast<const long long *>(wb.in_offsets);
    HIP_TRY(hipMemsetAsync(a.flag, 0, 8, s));
    LAUNCH_BLOCKS(lu_check_kernel, (b.N + 1 + 255) / 256, 256, 0, s, roff, (long long)b.N, (long long)b.total_bases, (long long)b.max_len,
                  (int)GENIE_MODE_BWA, 0, b.strands(), a.flag, static_cast<int32_t *>(nullptr), static_cast<long long *>(nullptr),
                  static_cast<long long *>(nullptr));
    if (in_off) LAUNCH_BLOCKS(chain_check_kernel, (U + 1 + 255) / 256, 256, 0, s, in_off, (long long)U, (long long)wb.in_total_rows, a.flag);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, a.flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return GENIE_E_INVALID;
    const LuReads R{b.bases, roff, (long long)b.N, b.strands()};
    const WinInput in{in_off, reinterpret_cast<const int4 *>(wb.in_rows), (long long)U, (int)wb.min_len};
    int4 *rows = reinterpret_cast<int4 *>(out.rows);
    long long *out_off = reinterpret_cast<long long *>(out.offsets);
    LAUNCH_BLOCKS(window_mark_kernel, (U + 255) / 256, 256, 0, s, ix->dev, R, in, reinterpret_cast<const int2 *>(wb.windows), a.win, a.has,
                  a.slot, a.cnt, a.added, a.st, b.status);
    if (int rc = launch_compact(a.has, reinterpret_cast<const int32_t *>(a.slot), U, 1, reinterpret_cast<int64_t *>(a.loff),
                                reinterpret_cast<int32_t *>(a.list), U, a.scan_tmp, stream))
        return rc;
    const long long most = (long long)(ix->num_cus > 0 ? ix->num_cus : 256) * 4;     // four waves per CU hold their tables in LDS
    const dim3 grid((unsigned)std::min<long long>(U, most));
    LAUNCH(window_wave_kernel<false>, grid, dim3(kWave), 0, s, ix->dev, R, in, static_cast<const long long *>(a.loff),
           static_cast<const int4 *>(a.list), static_cast<const int2 *>(a.win), a.cnt, a.added, a.st, b.status,
           static_cast<const long long *>(nullptr), static_cast<int4 *>(nullptr), 0ll);
    if (int rc = launch_compact(a.cnt, nullptr, U, 0x7fffffff, out.offsets, nullptr, 0, a.scan_tmp, stream)) return rc;
    if (rows && out.cap_rows > 0) {
        LAUNCH(window_wave_kernel<true>, grid, dim3(kWave), 0, s, ix->dev, R, in, static_cast<const long long *>(a.loff),
               static_cast<const int4 *>(a.list), static_cast<const int2 *>(a.win), a.cnt, a.added, a.st, b.status,
               static_cast<const long long *>(out_off), rows, (long long)out.cap_rows);
        if (in_off && wb.in_total_rows > 0)
            LAUNCH_BLOCKS(window_copy_kernel, (wb.in_total_rows + 255) / 256, 256, 0, s, in, static_cast<const int32_t *>(a.st),
                          static_cast<const long long *>(out_off), rows, (long long)out.cap_rows);
    }
    if (out.totals)
        LAUNCH(window_totals_kernel, dim3(1), dim3(kScanBlock), 0, s, static_cast<const int32_t *>(a.added),
               static_cast<const int32_t *>(a.st), static_cast<const long long *>(out_off), (long long)U,
               reinterpret_cast<long long *>(out.totals));
    return GENIE_OK;
}

// pairs.inc -- genie_pair_alignments: per pair of mates, which of their candidate records go together, the pair's mapping quality,
// and SAM's per-record fields of every record (included by align.inc behind select.inc, inside namespace genie).  The definition
// is the header's; DESIGN.md section 26 has the reasoning.
//
// Reads 2k and 2k + 1 are the mates of pair k.  The combinations of a pair are numbered c = x n1 + y over ALL its records, x the
// record of mate 0 and y that of mate 1, so (W descending, x ascending, y ascending) is (W descending, c ascending); those whose
// records are no candidates are passed over.  pair_decide is that program once, for one lane alone or for the 64 lanes of a wave:
//   PA0 chain_check_kernel  the record offsets; the host reads the flag: the call's one synchronisation
//   PA1 pair_lane_kernel    one lane per pair: marks the pairs of more than kPairLaneMax combinations as wide and decides the
//                           others, every record read from d_records
//   PA2 launch_compact      the wide pairs as a list (scan_block_sums_kernel)
//   PA3 pair_wave_kernel    one wave per wide pair, grid-stride over that list: lane l takes the combinations l, l + 64, ...; the
//                           (contig and strand, b, r_span, w) of the first kPairTile records of each mate in LDS, beyond it read
//                           back from d_records and d_class
//   PA4 pair_write_kernel   one lane per record: its d_sam row from its pair's d_pairs row, one 16-byte store
//   PA5 pair_totals_kernel  the four totals, by one block
// The best combination is an arg-max: the largest W over the wave, then the smallest c among the lanes that hold it (W takes 34
// bits and c up to 62, so the two do not share one 64-bit word).  W2 is one more reduction over each lane's two largest values.
namespace {

constexpr int kPairLaneMax = GENIE_PAIR_LANE_MAX;             // a pair of at most this many combinations is decided by one lane
constexpr int kPairTile = GENIE_PAIR_TILE;                    // records of a mate whose values live in LDS
constexpr int kPairWaves = 4;                                 // waves per block
constexpr int kPairNone = -1;                                 // the first word of a record that is no candidate
static_assert(kPairTile % kWave == 0 && 4 * kPairWaves * 2 * kPairTile * 16 <= 160 * 1024, "four blocks per CU");

struct PairParams {
    int orient, isize_min, isize_max, isize_mean, pen_slope, pen_max, pen_unpaired, mapq_boost;
};

struct PairInput {
    const long long *so;                  // d_sel_offsets
    long long N, P;
    const int4 *rec;                      // three to a record
    long long n_records;
    const int4 *klass;
    long long cap;
};

struct PairArea {
    int *flag;                            // PA0's verdict
    int32_t *wide, *pmapq;                // per pair: 1 for a wide pair; its mapping quality
    int4 *wslot, *wlist;                  // per pair: its index as a row, and the rows of the wide pairs
    long long *woff;                      // P + 1
    uint8_t *scan_tmp;                    // launch_compact's
};

inline int64_t pair_layout(uint8_t *base, int64_t P, PairArea *a)
{
    Carver c{base};
    c.take(a->flag, 8);
    c.take(a->wide, P * 4);
    c.take(a->pmapq, P * 4);
    c.take(a->wslot, P * 16);
    c.take(a->wlist, P * 16);
    c.take(a->woff, (P + 1) * 8);
    c.take(a->scan_tmp, compact_tmp_bytes(P));
    return c.at;
}

__device__ __forceinline__ long long pair_record_count(const PairInput &in) { return sel_clamp(in.so[in.N], 0, in.n_records); }

__device__ __forceinline__ int pair_clamp32(long long v) { return (int)sel_clamp(v, -0x7fffffffll - 1, 0x7fffffffll); }

// the records [lo, lo + n) of a read and the chain of its head
struct PairMate {
    int lo, n, head_chain;
};

__device__ __forceinline__ PairMate pair_mate(const PairInput &in, long long r)
{
    const long long R = pair_record_count(in);
    const long long a = sel_clamp(in.so[r], 0, R), b = sel_clamp(in.so[r + 1], a, R);
    return PairMate{(int)a, (int)(b - a), b > a ? in.rec[3 * a].y : -1};
}

// (contig and strand, b, r_span, w) of record j, whatever its kind
__device__ __forceinline__ int4 pair_values(const PairInput &in, long long j, int strand)
{
    const int4 r1 = in.rec[3 * j + 1];
    const int cs = (int)(((unsigned)r1.x << 1) | (strand != 0 ? 1u : 0u));
    return make_int4(cs, (int)((unsigned)r1.y - 1u), r1.z, in.rec[3 * j + 2].y);
}

// the same of record j as a record of mate m; kPairNone in .x unless it is the head or a secondary of the head
__device__ __forceinline__ int4 pair_cand(const PairInput &in, const PairMate &m, long long j)
{
    const int4 r0 = in.rec[3 * j];
    if (j != m.lo) {
        if (r0.z != kSelSecondary || in.cap <= 0) return make_int4(kPairNone, 0, 0, 0);
        if (in.klass[sel_clamp(r0.y, 0, in.cap - 1)].y != m.head_chain) return make_int4(kPairNone, 0, 0, 0);
    }
    return pair_values(in, j, r0.w);
}

struct PairCombo {
    long long W, span;
    int type;                             // 0 FR, 1 RF, 2 same strand, 3 none, -1 two contigs
    bool concordant;
};

__device__ __forceinline__ PairCombo pair_combo(const int4 &x, const int4 &y, const PairParams &p)
{
    PairCombo c{0, 0, -1, false};
    const unsigned d = (unsigned)x.x ^ (unsigned)y.x;
    if (d > 1u) return c;
    const long long bx = x.y, ex = bx + x.z, by = y.y, ey = by + y.z;
    c.span = (ex > ey ? ex : ey) - (bx < by ? bx : by);
    if (d == 0) {
        c.type = 2;
    } else {
        const bool xf = (x.x & 1) == 0;
        const long long fb = xf ? bx : by, fe = xf ? ex : ey, rb = xf ? by : bx, re = xf ? ey : ex;
        c.type = (fb <= rb && fe <= re) ? 0 : ((rb <= fb && re <= fe) ? 1 : 3);
    }
    c.concordant = c.type != 3 && ((p.orient >> c.type) & 1) != 0 && c.span >= p.isize_min && c.span <= p.isize_max;
    const long long off = c.span > p.isize_mean ? c.span - p.isize_mean : (long long)p.isize_mean - c.span;
    const long long pen = off * p.pen_slope / 256;
    c.W = (long long)x.w + y.w - (pen < p.pen_max ? pen : p.pen_max);
    return c;
}

__device__ __forceinline__ unsigned long long pair_biased(long long v) { return (unsigned long long)v ^ 0x8000000000000000ull; }

__device__ __forceinline__ long long pair_wave_max(long long v) { return (long long)pair_biased((long long)chain_wave_max64(pair_biased(v))); }

constexpr long long kPairLeast = -0x7fffffffffffffffll - 1;   // below every W

// One pair.  kWide: the 64 lanes of a wave, lane l taking the combinations l, l + 64, ... and `tile` holding the values of the
// first min(n, kPairTile) records of mate 0 and, kPairTile further on, of mate 1; else one lane alone.
template <bool kWide>
__device__ __forceinline__ void pair_decide(const PairInput &in, const PairParams &p, const PairMate &m0, const PairMate &m1, int lane,
                                            const int4 *tile, int4 *__restrict__ pairs, int32_t *__restrict__ pmapq)
{
    const int nt0 = kWide ? (m0.n < kPairTile ? m0.n : kPairTile) : 0, nt1 = kWide ? (m1.n < kPairTile ? m1.n : kPairTile) : 0;
    const long long total = (long long)m0.n * m1.n;
    long long best = kPairLeast, second = kPairLeast, best_c = -1, ncon = 0;
    if (kWide) {
        unsigned x = (unsigned)(lane / (unsigned)m1.n), y = (unsigned)(lane % (unsigned)m1.n), last_x = 0xffffffffu;
        int4 vx = make_int4(kPairNone, 0, 0, 0);
        for (long long c = lane; c < total; c += kWave) {
            if (x != last_x) {
                vx = (int)x < nt0 ? tile[x] : pair_cand(in, m0, (long long)m0.lo + x);
                last_x = x;
            }
            if (vx.x != kPairNone) {
                const int4 vy = (int)y < nt1 ? tile[kPairTile + y] : pair_cand(in, m1, (long long)m1.lo + y);
                if (vy.x != kPairNone) {
                    const PairCombo k = pair_combo(vx, vy, p);
                    if (k.concordant) {
                        ncon++;
                        if (k.W > best) {
                            second = best;
                            best = k.W;
                            best_c = c;
                        } else if (k.W > second) {
                            second = k.W;
                        }
                    }
                }
            }
            y += kWave;
            x += y / (unsigned)m1.n;
            y %= (unsigned)m1.n;
        }
    } else {
        for (int x = 0; x < m0.n; x++) {
            const int4 vx = pair_cand(in, m0, (long long)m0.lo + x);
            if (vx.x == kPairNone) continue;
            for (int y = 0; y < m1.n; y++) {
                const int4 vy = pair_cand(in, m1, (long long)m1.lo + y);
                if (vy.x == kPairNone) continue;
                const PairCombo k = pair_combo(vx, vy, p);
                if (!k.concordant) continue;
                ncon++;
                if (k.W > best) {
                    second = best;
                    best = k.W;
                    best_c = (long long)x * m1.n + y;
                } else if (k.W > second) {
                    second = k.W;
                }
            }
        }
    }
    long long W1 = best, c1 = best_c, W2 = second;
    if (kWide) {
        ncon = (long long)wave_sum64((unsigned long long)ncon);
        W1 = pair_wave_max(best);
        // the smallest c among the lanes that hold W1: c is below 2^62, so its complement orders them
        c1 = (long long)~chain_wave_max64(best == W1 && best_c >= 0 ? ~(unsigned long long)best_c : 0ull);
        W2 = pair_wave_max(best == W1 && best_c == c1 ? second : best);
    }
    if (kWide && lane != 0) return;
    const bool has0 = m0.n > 0, has1 = m1.n > 0, any = ncon > 0;
    if (!any) W1 = 0;
    if (ncon < 2) W2 = 0;
    int4 h0 = make_int4(kPairNone, 0, 0, 0), h1 = h0;
    if (has0) h0 = pair_values(in, m0.lo, in.rec[3 * (long long)m0.lo].w);
    if (has1) h1 = pair_values(in, m1.lo, in.rec[3 * (long long)m1.lo].w);
    const long long U = (long long)h0.w + h1.w - p.pen_unpaired;
    const bool proper = has0 && has1 && any && W1 >= U;
    int mapq = 0, rec0 = has0 ? m0.lo : -1, rec1 = has1 ? m1.lo : -1;
    int4 v0 = h0, v1 = h1;
    if (proper) {
        long long floor_ = W2 > U ? W2 : U;
        floor_ = floor_ > 0 ? floor_ : 0;
        floor_ = floor_ < W1 ? floor_ : W1;
        mapq = W1 <= 0 ? 0 : (int)(60 * (W1 - floor_) / W1);
        rec0 = m0.lo + (int)(c1 / m1.n);
        rec1 = m1.lo + (int)(c1 % m1.n);
        v0 = pair_values(in, rec0, in.rec[3 * (long long)rec0].w);
        v1 = pair_values(in, rec1, in.rec[3 * (long long)rec1].w);
    }
    int isize = 0, type = -1;
    if (has0 && has1) {
        const PairCombo k = pair_combo(v0, v1, p);
        if (k.type >= 0) {
            isize = pair_clamp32(k.span);
            type = k.type;
        }
    }
    const int flags = (proper ? 1 : 0) | (has0 ? 2 : 0) | (has1 ? 4 : 0) | (has0 && rec0 != m0.lo ? 8 : 0) | (has1 && rec1 != m1.lo ? 16 : 0);
    pairs[0] = make_int4(rec0, rec1, flags, pair_clamp32(W1));
    pairs[1] = make_int4(pair_clamp32(W2), isize, (int)(ncon < 0x7fffffffll ? ncon : 0x7fffffffll), type);
    *pmapq = mapq;
}

__global__ void __launch_bounds__(256) pair_lane_kernel(PairInput in, PairParams p, int4 *__restrict__ pairs, int32_t *__restrict__ pmapq,
                                                        int32_t *__restrict__ wide, int4 *__restrict__ wslot)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.P) return;
    const PairMate m0 = pair_mate(in, 2 * i), m1 = pair_mate(in, 2 * i + 1);
    const bool w = (long long)m0.n * m1.n > kPairLaneMax;
    wide[i] = w ? 1 : 0;
    wslot[i] = make_int4((int)i, 0, 0, 0);
    if (w) return;                                                   // PA3 decides it
    pair_decide<false>(in, p, m0, m1, 0, nullptr, pairs + 2 * i, pmapq + i);
}

__global__ void __launch_bounds__(kPairWaves *kWave) pair_wave_kernel(PairInput in, PairParams p, const long long *__restrict__ woff,
                                                                      const int4 *__restrict__ wlist, int4 *__restrict__ pairs,
                                                                      int32_t *__restrict__ pmapq)
{
    __shared__ int4 tiles[kPairWaves][2 * kPairTile];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int4 *tile = tiles[wave];
    const long long nw = sel_clamp(woff[in.P], 0, in.P);
    for (long long k = (long long)blockIdx.x * kPairWaves + wave; k < nw; k += (long long)gridDim.x * kPairWaves) {
        const long long i = sel_clamp(wlist[k].x, 0, in.P - 1);
        const PairMate m0 = pair_mate(in, 2 * i), m1 = pair_mate(in, 2 * i + 1);
        if ((long long)m0.n * m1.n <= 0) continue;                   // not a wide pair: nothing to divide by
        wave_lds_fence();                                            // the pair before has read the tile
        for (int j = lane; j < m0.n && j < kPairTile; j += kWave) tile[j] = pair_cand(in, m0, (long long)m0.lo + j);
        for (int j = lane; j < m1.n && j < kPairTile; j += kWave) tile[kPairTile + j] = pair_cand(in, m1, (long long)m1.lo + j);
        wave_lds_fence();
        pair_decide<true>(in, p, m0, m1, lane, tile, pairs + 2 * i, pmapq + i);
    }
}

__global__ void __launch_bounds__(256) pair_write_kernel(PairInput in, PairParams p, const int4 *__restrict__ pairs,
                                                         const int32_t *__restrict__ pmapq, int4 *__restrict__ sam)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= pair_record_count(in)) return;
    long long lo = 0, hi = in.N;                                     // the last r in [0, N) with so[r] <= j
    while (lo < hi - 1) {
        const long long mid = (lo + hi) >> 1;
        if (in.so[mid] <= j) lo = mid; else hi = mid;
    }
    const long long k = lo >> 1;
    const int m = (int)(lo & 1);
    const int4 pr = pairs[2 * k];
    const long long R = pair_record_count(in);
    const int mine = m ? pr.y : pr.x;
    int mate = m ? pr.x : pr.y;
    mate = mate >= 0 && mate < R ? mate : -1;
    const bool proper = (pr.z & 1) != 0;
    const int4 r0 = in.rec[3 * j];
    const int4 v = pair_values(in, j, r0.w);
    int flag = 1 | (proper ? 2 : 0) | ((v.x & 1) ? 0x10 : 0) | (m ? 0x80 : 0x40), tlen = 0;
    if (mate < 0) {
        flag |= 8;
    } else {
        const int4 w = pair_values(in, mate, in.rec[3 * (long long)mate].w);
        if (w.x & 1) flag |= 0x20;
        if (((unsigned)v.x ^ (unsigned)w.x) <= 1u) {
            const long long bv = v.y, ev = bv + v.z, bw = w.y, ew = bw + w.z;
            const long long span = (ev > ew ? ev : ew) - (bv < bw ? bv : bw);
            const bool left = bv < bw || (bv == bw && m == 0);
            tlen = pair_clamp32(left ? span : -span);
        }
    }
    int mapq = 0;
    if (j == mine) {
        const int q = (int)sel_clamp(in.rec[3 * j + 2].w, 0, 60);
        const int up = pmapq[k] < q + p.mapq_boost ? pmapq[k] : q + p.mapq_boost;
        mapq = proper && up > q ? up : q;
        if (r0.z == kSelSupp) flag |= 0x800;
    } else if (r0.z == kSelSupp) {
        flag |= 0x800;
        mapq = in.rec[3 * j + 2].w;
    } else {
        flag |= 0x100;
    }
    sam[j] = make_int4(flag, mapq, mate, tlen);
}

// {pairs with both mates mapped, proper pairs, mates whose chosen record is not their head, pairs with one mate mapped}, by one block
__global__ void __launch_bounds__(kScanBlock) pair_totals_kernel(const int4 *__restrict__ pairs, long long P, long long *__restrict__ totals)
{
    __shared__ unsigned long long wsum[4][kScanBlock / kWave];
    unsigned long long a = 0, b = 0, c = 0, d = 0;
    for (long long i = threadIdx.x; i < P; i += kScanBlock) {
        const int f = pairs[2 * i].z;
        a += (f & 6) == 6 ? 1u : 0u;
        b += (unsigned)(f & 1);
        c += (unsigned)((f >> 3) & 1) + (unsigned)((f >> 4) & 1);
        d += (f & 6) == 2 || (f & 6) == 4 ? 1u : 0u;
    }
    a = wave_sum64(a);
    b = wave_sum64(b);
    c = wave_sum64(c);
    d = wave_sum64(d);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        wsum[0][threadIdx.x / kWave] = a;
        wsum[1][threadIdx.x / kWave] = b;
        wsum[2][threadIdx.x / kWave] = c;
        wsum[3][threadIdx.x / kWave] = d;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long all = 0;
        for (int w = 0; w < kScanBlock / kWave; w++) all += wsum[threadIdx.x][w];
        totals[threadIdx.x] = (long long)all;
    }
}

}  // namespace

int64_t pair_alignments_workspace_bytes(int64_t N, int64_t n_records)
{
    (void)n_records;                                                 // nothing is kept per record
    PairArea a;
    return pair_layout(nullptr, N / 2, &a);
}

int launch_pair_alignments(const genie_index *ix, const PairBatch &b, const PairOut &out, void *ws, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = b.N, P = N / 2, n_rec = b.n_records;
    if (N == 0) {
        if (out.totals) HIP_TRY(hipMemsetAsync(out.totals, 0, 32, s));
        return GENIE_OK;
    }
    PairArea a;
    pair_layout(static_cast<uint8_t *>(ws), P, &a);
    const long long *so = reinterpret_cast<const long long *>(b.sel_offsets);
    HIP_TRY(hipMemsetAsync(a.flag, 0, 8, s));
    LAUNCH_BLOCKS(chain_check_kernel, (N + 1 + 255) / 256, 256, 0, s, so, (long long)N, 0x7fffffffffffffffll, a.flag);
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, a.flag, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) return GENIE_E_INVALID;
    const PairInput in{so, (long long)N, (long long)P, reinterpret_cast<const int4 *>(b.records), (long long)n_rec,
                       reinterpret_cast<const int4 *>(b.klass), (long long)b.cap_chains};
    const PairParams p{b.orient, b.isize_min, b.isize_max, b.isize_mean, b.pen_slope, b.pen_max, b.pen_unpaired, b.mapq_boost};
    int4 *pairs = reinterpret_cast<int4 *>(out.pairs);
    LAUNCH_BLOCKS(pair_lane_kernel, (P + 255) / 256, 256, 0, s, in, p, pairs, a.pmapq, a.wide, a.wslot);
    const long long wide_most = std::min<long long>(P, n_rec / 17);                  // 8 x 9: a wide pair has at least 17 records
    if (wide_most > 0) {
        if (int rc = launch_compact(a.wide, reinterpret_cast<const int32_t *>(a.wslot), P, 1, reinterpret_cast<int64_t *>(a.woff),
                                    reinterpret_cast<int32_t *>(a.wlist), P, a.scan_tmp, stream))
            return rc;
        const long long want = (wide_most + kPairWaves - 1) / kPairWaves, most = (long long)(ix->num_cus > 0 ? ix->num_cus : 256) * 4;
        LAUNCH(pair_wave_kernel, dim3((unsigned)std::min(want, most)), dim3(kPairWaves * kWave), 0, s, in, p,
               static_cast<const long long *>(a.woff), static_cast<const int4 *>(a.wlist), pairs, a.pmapq);
    }
    if (n_rec > 0)
        LAUNCH_BLOCKS(pair_write_kernel, (n_rec + 255) / 256, 256, 0, s, in, p, static_cast<const int4 *>(pairs),
                      static_cast<const int32_t *>(a.pmapq), reinterpret_cast<int4 *>(out.sam));
    if (out.totals)
        LAUNCH(pair_totals_kernel, dim3(1), dim3(kScanBlock), 0, s, static_cast<const int4 *>(pairs), (long long)P,
               reinterpret_cast<long long *>(out.totals));
    return GENIE_OK;
}

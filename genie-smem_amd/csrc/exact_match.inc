// exact_match.inc -- genie_exact_match: the suffix-array interval of every pattern of a CSR batch, both strands if asked
// (included by kernels.hip behind long_units.inc, inside namespace genie).
//
// A pattern is a unit of long_units.inc that is searched whole.  The front is lu_run's as it stands: LU0 checks the offsets
// on the device (mode BWA: no pattern is too short) and, on two strands, writes the strand table.  SPLIT_BREAKS is never
// given, so only tail.empty() and tail.whole() are reached.  The tail:
//   LR1 lr_pack_kernel      the packed stream of the strand-patterns (a reversed one is read backwards and complemented: the
//                           reverse complement never exists as bytes); a code > 3 is the strand-pattern's status
//   EM  exact_match_kernel  one LANE per strand-pattern: sa_interval over its words of the stream (QPlain, any length), the
//                           directory read from global memory (ix.dir); interval, count and status leave with non-temporal
//                           vector stores.  Nothing is shared between lanes and no atomic decides a value.
// When the caller's max_len is at most kEmDirect there is no LR1: exact_match_kernel<true> has every lane pack its own
// pattern from the caller's bytes into two registers (QTwo) -- the same reading rule, backwards and complemented for a
// reversed one -- and find the bad base itself.  LR1 spends a thread, a bisection of the offsets and three padding words
// on every word of the stream, which for such patterns is most of the call (DESIGN.md section 16).
// The workspace is lu_run's layout without fwd[] (kFwd false): flag block, statuses, the packed stream and, on two strands,
// the strand table.
namespace {

constexpr int kEmBlock = 256;
constexpr int kEmDirect = 64;             // bases that two 64-bit words hold

// a pattern of at most 64 bases in two registers, zero padded as the stream is
struct QTwo {
    uint64_t w0, w1;
    __device__ __forceinline__ uint64_t win(int pos) const
    {
        const int sh = (pos & 31) * 2;
        return (pos >> 5) ? funnel(w1, 0ull, sh) : funnel(w0, w1, sh);
    }
};

// usrc[q]: as lr_pack_kernel's (null: forward, from byte uoff[q]).  DIRECT: every pattern has at most kEmDirect bases (LU0 has
// checked the caller's max_len on the device before this kernel is launched); packed and st are not read.
template <bool DIRECT>
__global__ void __launch_bounds__(kEmBlock) exact_match_kernel(DevIndex ix, const uint8_t *__restrict__ bases,
                                                               const long long *__restrict__ uoff, const long long *__restrict__ usrc,
                                                               long long U, const uint64_t *__restrict__ packed,
                                                               const int32_t *__restrict__ st, int2 *__restrict__ lohi,
                                                               int32_t *__restrict__ counts, int32_t *__restrict__ status)
{
    const long long q = (long long)blockIdx.x * kEmBlock + threadIdx.x;
    if (q >= U) return;
    const long long o = uoff[q];
    const int L = (int)(uoff[q + 1] - o);
    int2 iv = make_int2(-2, -2);
    bool bad;
    if (DIRECT) {
        const long long key = usrc ? usrc[q] : 2 * o;
        const bool rev = key & 1;
        const uint8_t *src = bases + (key >> 1);
        const uint32_t flip = rev ? 3u : 0u;
        uint64_t w0 = 0, w1 = 0;
        uint32_t any = 0;
        for (int j = 0; j < L; j++) {
            const uint32_t c = rev ? src[-j] : src[j];
            any |= c;
            const uint64_t code = (uint64_t)((c & 3u) ^ flip) << (62 - 2 * (j & 31));
            if (j < 32) w0 |= code; else w1 |= code;
        }
        bad = any > 3u;
        if (!bad) iv = sa_interval(ix, ix.dir, QTwo{w0, w1}, 0, L);
    } else {
        bad = st[q] == GENIE_READ_BAD_BASE;
        if (!bad) iv = sa_interval(ix, ix.dir, QPlain{packed + lr_wd(uoff, q)}, 0, L);
    }
    lr_store_lohi(lohi + q, iv);
    if (counts) __builtin_nontemporal_store(iv.x >= 0 ? iv.y - iv.x + 1 : 0, counts + q);
    if (status) __builtin_nontemporal_store(bad ? (int32_t)GENIE_READ_BAD_BASE : (int32_t)GENIE_READ_OK, status + q);
}

struct LuExactTail {
    static constexpr bool kSmems = false, kFwd = false;
    const genie_index *ix;
    const CsrBatch &b;
    int32_t *d_lohi, *d_counts;
    hipStream_t s;

    int empty() { return GENIE_OK; }
    int whole(const LongArea &lr, const long long *uoff, const long long *usrc)
    {
        const long long SN = b.strand_reads();
        const bool direct = b.max_len <= kEmDirect;
        if (!direct)
            LAUNCH_BLOCKS(lr_pack_kernel, (lr.nwords + 255) / 256, 256, 0, s, b.bases, uoff, SN, usrc, lr.nwords,
                   lr.packed, lr.st);
        const auto kernel = direct ? exact_match_kernel<true> : exact_match_kernel<false>;
        LAUNCH_BLOCKS(kernel, (SN + kEmBlock - 1) / kEmBlock, kEmBlock, 0, s, ix->dev, b.bases, uoff, usrc, SN,
               static_cast<const uint64_t *>(lr.packed), static_cast<const int32_t *>(lr.st), reinterpret_cast<int2 *>(d_lohi),
               d_counts, b.status);
        return GENIE_OK;
    }
    int broken(long long) { return GENIE_E_INVALID; }            // not reached: SPLIT_BREAKS is refused by the C ABI
    int pass(const LuPass &) { return GENIE_E_INVALID; }
};

}  // namespace

int64_t exact_match_workspace_bytes(int64_t N, int64_t total_bases, int32_t flags)
{
    return long_ex_bytes(N, total_bases, flags, false, false);
}

int launch_exact_match(const genie_index *ix, const CsrBatch &b, int32_t *d_lohi, int32_t *d_counts, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    LuExactTail tail{ix, b, d_lohi, d_counts, s};
    return lu_run(ix, GENIE_MODE_BWA, b, s, tail);
}

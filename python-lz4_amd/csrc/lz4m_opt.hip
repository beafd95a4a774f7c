// lz4m_opt.hip -- price-based optimal parse of LZ4 blocks for MI355X (gfx950):
// lz4.block.compress(mode="optimal"), batched (lz4m_compress_opt_batch).
//
// A valid LZ4 block for every input, within 1 % of LZ4_compress_HC(12) on
// compressible data at level 9 (DESIGN.md section 9.7 has the measured sizes),
// NOT byte-identical to lz4hc.c.  The parse is defined serially in DESIGN.md
// section 9.7 and restated on the CPU by tests/hc_model/opt_model.c; these
// kernels produce that model's bytes:
//   - section 9.1's tables (13-bit hash, chain of distances <= 65535) and
//     level table (`attempts`): lz4m_chain.h, shared with lz4m_hc.hip;
//   - L[q], O[q]: the longest forward match among the first `attempts` chain
//     candidates of q (q <= n - 12), at most min(n - 5 - q, 65535) bytes, the
//     nearest among equals;
//   - cost[p], backwards from cost[n] = 1: a literal (cost[p + 1] + 1, + 1
//     where the literal run's length needs another byte) against the cheapest
//     of the 64 matches of L[p] .. max(4, L[p] - 63) bytes (3 + length bytes +
//     cost[p + ml]); the longest among equal matches, a match before a literal;
//   - the choices followed from 0; the block is cost[0] bytes, written only
//     if that fits.
//
// Mapping: one wavefront per block, a persistent grid striding over the batch,
// the block's state in the wave's slice of the caller's workspace (10 bytes
// per position: u32 L|O<<16, u32 cost, u16 chain).  Four phases per block:
//   insert  64 positions per step, linked by ballots (hc_insert_step); the head
//           table is the workgroup's LDS.  chain[q] is then the distance to
//           the newest earlier position with q's hash;
//   match   64 consecutive positions per step, each lane walking its own chain
//           for `attempts` candidates and counting forwards 8 bytes at a time.
//           The match of the step's predecessor position, less the bytes up to
//           a lane's position, is known to hold at the same distance and is
//           not counted again, so a long run costs its length once;
//   price   the backward pass, 32 positions per chunk.  A run of positions
//           without a match is one vector step (closed form).  A position with
//           one is one wave-step: lane k prices length L - k, reading cost[p +
//           L - k] from a ring of the last 1024 costs in LDS (the head table's
//           memory, free by now); a wave minimum and a ballot pick the length.
//           Matches of >= 575 bytes reach past the ring: their 64 costs are
//           final long before, and their addresses depend on L alone, so they
//           are loaded from the workspace a chunk ahead (with L itself two
//           chunks ahead) and staged in LDS: no global load waits on the
//           chain of prices;
//   emit    forwards over the choices, 64 positions per look.
// No phase reads workspace bytes the block did not write, so a block's bytes
// do not depend on the wave that parsed it or on what the workspace held.
#include "lz4m_chain.h"

#include "../../include/lz4m.h"

namespace lz4m {
namespace {

constexpr int32_t kOptMaxLen = 65535;     // longest match (u16 L)
constexpr int kOptLengths = 64;           // K: lengths priced per position, one per lane
constexpr int kOptChunk = 32;             // positions per price chunk
constexpr int kOptRing = 1024;            // costs kept in LDS
constexpr int32_t kOptFar = 512 + kOptLengths - 1;   // L from which all 64 costs lie >= 512 positions ahead
constexpr size_t kOptPosBytes = 10;       // workspace bytes per position
static_assert(kOptLengths == kWave, "one length per lane");
static_assert((kOptRing + kOptChunk * kWave) * 4 <= kHcHeads * 2, "ring and staging fit the smaller head table");
static_assert(kOptFar < kOptRing && kOptFar - kOptLengths + 1 >= 2 * kOptChunk, "near costs in the ring, far ones final");

// positions a block of n bytes holds in its slice (cost[n] included)
__host__ __device__ __forceinline__ int64_t opt_positions(int64_t n) { return (n + 64) & ~(int64_t)63; }

typedef __attribute__((address_space(3))) uint32_t lds_u32;

// One block by one wave; all arguments uniform.  Returns the block's size, or
// 0 if it does not fit in cap.
template <bool BIG>
__device__ __forceinline__ int32_t opt_block(__attribute__((address_space(3))) typename HcCfg<BIG ? kHcBig : kHcSmall>::head_t* head,
                                             uint8_t* slice, const uint8_t* src, int32_t n, uint8_t* dst,
                                             int32_t cap, int32_t attempts, uint32_t lane) {
    int32_t op = 0;
    if (n < 13) return hc_emit(dst, op, cap, src, 0, n, 0, 0, lane) ? op : 0;
    const int64_t np = opt_positions(n);
    uint32_t* lo = (uint32_t*)slice;            // L | O << 16; after pricing the chosen length | O << 16
    uint32_t* cost = lo + np;
    uint16_t* chain = (uint16_t*)(cost + np);
    const int32_t mflimit = n - 12, ilimit = n - 11;

    // ---- insert
    for (int32_t i = (int32_t)lane; i < kHcHeads; i += kWave) hc_st(head + i, 0u);
    hc_fence();
    for (int32_t base = 0; base < ilimit; base += kWave)
        hc_insert_step<false, kNoMask>(head, chain, src, base, ilimit, lane);

    // ---- match
    int32_t Lb = 0, Ob = 0;   // L and O of the position before the step's first
    for (int32_t base = 0; base < n; base += kWave) {
        const int32_t q = base + (int32_t)lane;
        int32_t bestL = 0, bestO = 0;
        if (q <= mflimit) {
            const int32_t lim = n - 5 - q < kOptMaxLen ? n - 5 - q : kOptMaxLen;
            const int32_t known = Lb - 1 - (int32_t)lane;   // bytes known equal at distance Ob (<= lim)
            const uint32_t want = ld32(src + q);
            uint32_t at = 0;   // src[q + bestL] once a match is held
            uint32_t d = hc_ld(chain + q);
            int32_t c = q;
            for (int32_t left = attempts; left > 0 && d != 0; --left) {
                c -= (int32_t)d;
                if (c < 0 || q - c > kHcMaxDist) break;
                d = hc_ld(chain + c);   // the next candidate: requested before this one is measured
                // one load decides most candidates: a match has q's first four bytes, and a longer one
                // than the best so far (bestL < lim here) also the byte that follows the best
                const bool open = bestL == 0 ? ld32(src + c) == want : src[c + bestL] == at;
                if (!open) continue;
                const int32_t start = (q - c == Ob && known > 0) ? known : 0;
                const int32_t fwd = start + hc_count(src + c + start, src + q + start, lim - start);
                if (fwd > bestL) {   // (>= 4: the first four bytes are equal)
                    bestL = fwd;
                    bestO = q - c;
                    if (fwd == lim) break;   // nothing longer exists
                    at = src[q + fwd];
                }
            }
        }
        if (q < n) hc_st(lo + q, (uint32_t)bestL | ((uint32_t)bestO << 16));
        Lb = rdl(bestL, kWave - 1);
        Ob = rdl(bestO, kWave - 1);
    }
    hc_fence();

    // ---- price (the head table's LDS now holds the ring and the staged far costs)
    lds_u32* ring = (lds_u32*)head;
    lds_u32* stage = ring + kOptRing;
    if (lane == 0) {
        hc_st(ring + ((uint32_t)n & (kOptRing - 1)), 1u);
        hc_st(cost + n, 1u);
    }
    hc_fence();
    int32_t lit = 0, cnext = 1;   // lit[p + 1], cost[p + 1]
    int32_t cb = (n - 1) & ~(kOptChunk - 1);
    auto load_lo = [&](int32_t b) __attribute__((always_inline)) {
        return (b >= 0 && lane < (uint32_t)kOptChunk && b + (int32_t)lane < n) ? hc_ld(lo + b + (int32_t)lane) : 0u;
    };
    uint32_t cur = load_lo(cb), nxt = load_lo(cb - kOptChunk);
    while (cb >= 0) {
        const int32_t nb = cb - kOptChunk;
        const uint32_t nxt2 = load_lo(nb - kOptChunk);
        // the next chunk's far costs: requested now, staged after this chunk
        const uint64_t farm = __ballot((int32_t)(nxt & 0xFFFFu) >= kOptFar);
        uint32_t far[kOptChunk];
#pragma unroll
        for (int j = 0; j < kOptChunk; ++j) {
            far[j] = 0;
            if ((farm >> j) & 1ull) far[j] = hc_ld(cost + nb + j + rdl((int32_t)(nxt & 0xFFFFu), j) - (int32_t)lane);
        }
        const uint64_t mt = __ballot((cur & 0xFFFFu) != 0);
        int32_t j = n - 1 - cb < kOptChunk - 1 ? n - 1 - cb : kOptChunk - 1;
        while (j >= 0) {
            if (!((mt >> j) & 1ull)) {   // a run of positions without a match: j down to j0
                const uint64_t m = mt & ((2ull << j) - 1ull);
                const int32_t j0 = m ? 64 - (int32_t)__builtin_clzll(m) : 0;
                const int32_t r = j - j0 + 1;
                const int32_t e0 = ext_len<BIG>(lit);
                if ((int32_t)lane < r) {
                    const int32_t p = cb + j - (int32_t)lane;
                    const int32_t l = lit + (int32_t)lane + 1;
                    const uint32_t c = (uint32_t)(cnext + (int32_t)lane + 1 + ext_len<BIG>(l) - e0);
                    hc_st(ring + ((uint32_t)p & (kOptRing - 1)), c);
                    hc_st(cost + p, c);
                }
                cnext += r + ext_len<BIG>(lit + r) - e0;
                lit += r;
                j = j0 - 1;
            } else {
                const int32_t p = cb + j;
                const uint32_t w = (uint32_t)rdl((int32_t)cur, j);
                const int32_t L = (int32_t)(w & 0xFFFFu);
                const int32_t ml = L - (int32_t)lane;
                const bool valid = ml >= 4;
                uint32_t v = 0;
                if (valid)
                    v = L >= kOptFar ? hc_ld(stage + j * kWave + (int32_t)lane)
                                     : hc_ld(ring + ((uint32_t)(p + ml) & (kOptRing - 1)));
                const int32_t inv = valid ? 0x7FFFFFFF - (3 + ext_len<BIG>(ml - 4) + (int32_t)v) : 0;
                const int32_t top = wave_max(inv);
                const int kk = __builtin_ctzll(__ballot(valid && inv == top));   // the longest of the cheapest
                const int32_t mc = 0x7FFFFFFF - top;
                const int32_t lc = cnext + 1 + ext_len<BIG>(lit + 1) - ext_len<BIG>(lit);
                int32_t c, choice;
                if (mc <= lc) {
                    c = mc;
                    choice = L - kk;
                    lit = 0;
                } else {
                    c = lc;
                    choice = 0;
                    lit += 1;
                }
                if (lane == 0) {
                    hc_st(ring + ((uint32_t)p & (kOptRing - 1)), (uint32_t)c);
                    hc_st(cost + p, (uint32_t)c);
                    hc_st(lo + p, (w & 0xFFFF0000u) | (uint32_t)choice);
                }
                cnext = c;
                --j;
            }
            hc_fence();
        }
#pragma unroll
        for (int j2 = 0; j2 < kOptChunk; ++j2)
            if ((farm >> j2) & 1ull) hc_st(stage + j2 * kWave + (int32_t)lane, far[j2]);
        hc_fence();
        cur = nxt;
        nxt = nxt2;
        cb = nb;
    }

    // ---- emit: cnext is cost[0], the block's size
    if (cnext > cap) return 0;
    int32_t p = 0, anchor = 0;
    while (p < n) {
        const int32_t q = p + (int32_t)lane;
        const uint32_t w = q < n ? hc_ld(lo + q) : 0u;
        const uint64_t m = __ballot((w & 0xFFFFu) != 0);
        if (m == 0) {
            p += kWave;
            continue;
        }
        const int f = __builtin_ctzll(m);
        const uint32_t ww = (uint32_t)rdl((int32_t)w, f);
        const int32_t ml = (int32_t)(ww & 0xFFFFu), s = p + f;
        if (!hc_emit(dst, op, cap, src, anchor, s - anchor, (int32_t)(ww >> 16), ml, lane)) return 0;
        p = s + ml;
        anchor = p;
    }
    if (!hc_emit(dst, op, cap, src, anchor, n - anchor, 0, 0, lane)) return 0;
    return op;
}

// The persistent grid: wave blockIdx.x takes every gridDim.x-th block of the
// batch and parses those of its own configuration (BIG: longer than 64 KiB).
// A block whose state does not fit the wave's slice reports 0.
template <bool BIG>
__global__ __launch_bounds__(64) void opt_parse_kernel(const uint8_t* __restrict__ src_base,
                                                       const int64_t* __restrict__ src_off,
                                                       const int32_t* __restrict__ src_len,
                                                       uint8_t* __restrict__ dst_base,
                                                       const int64_t* __restrict__ dst_off,
                                                       const int32_t* __restrict__ dst_cap,
                                                       int32_t* __restrict__ out_len, int64_t nblocks,
                                                       int32_t attempts, uint8_t* __restrict__ work,
                                                       uint64_t slice_bytes) {
    typedef typename HcCfg<BIG ? kHcBig : kHcSmall>::head_t head_mem_t;
    __shared__ __attribute__((aligned(16))) head_mem_t head_mem[kHcHeads];
    const uint32_t lane = threadIdx.x;
    uint8_t* slice = work + (size_t)blockIdx.x * slice_bytes;
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int32_t n = src_len[b];
        if ((n > kHcSmallMax) != BIG) continue;   // the other kernel's block (a negative n is refused here)
        const int32_t cap = dst_cap[b];
        if (n < 0 || n > kHcMaxInput || cap < 0 || (uint64_t)opt_positions(n) * kOptPosBytes > slice_bytes) {
            if (lane == 0) out_len[b] = 0;
            continue;
        }
        const int32_t r = opt_block<BIG>((__attribute__((address_space(3))) head_mem_t*)head_mem, slice,
                                         src_base + src_off[b], n, dst_base + dst_off[b], cap, attempts, lane);
        if (lane == 0) out_len[b] = r;
    }
}

}  // namespace
}  // namespace lz4m

extern "C" size_t lz4m_compress_opt_workspace_size(int64_t n, int32_t max_len) {
    using namespace lz4m;
    if (n <= 0 || max_len < 0) return 0;
    const int64_t waves = n < HcCfg<kHcSmall>::kWaves ? n : HcCfg<kHcSmall>::kWaves;
    return (size_t)waves * (size_t)opt_positions(max_len) * kOptPosBytes;
}

extern "C" int lz4m_compress_opt_batch(const uint8_t* d_src, const int64_t* d_src_off, const int32_t* d_src_len,
                                       uint8_t* d_dst, const int64_t* d_dst_off, const int32_t* d_dst_cap,
                                       int32_t* d_out_len, int64_t n, int level, void* d_work, size_t work_bytes,
                                       lz4m_stream_t stream) {
    using namespace lz4m;
    if (n < 0) return LZ4M_EINVAL;
    if (n == 0) return 0;
    if (d_work == nullptr || ((uintptr_t)d_work & 3u) || work_bytes < lz4m_compress_opt_workspace_size(n, 0))
        return LZ4M_EINVAL;
    const int32_t attempts = hc_attempts(level);
    hipStream_t st = (hipStream_t)stream;
    // one slice per wave of the wider grid, a multiple of 64 positions; both
    // kernels walk the whole batch and take their own blocks
    const uint32_t small_grid = (uint32_t)(n < HcCfg<kHcSmall>::kWaves ? n : HcCfg<kHcSmall>::kWaves);
    const uint64_t unit = 64 * kOptPosBytes;
    const uint64_t slice_bytes = (uint64_t)work_bytes / small_grid / unit * unit;
    hipLaunchKernelGGL(opt_parse_kernel<false>, dim3(small_grid), dim3(64), 0, st, d_src, d_src_off, d_src_len, d_dst,
                       d_dst_off, d_dst_cap, d_out_len, n, attempts, (uint8_t*)d_work, slice_bytes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const uint32_t big_grid = (uint32_t)(n < HcCfg<kHcBig>::kWaves ? n : HcCfg<kHcBig>::kWaves);
    hipLaunchKernelGGL(opt_parse_kernel<true>, dim3(big_grid), dim3(64), 0, st, d_src, d_src_off, d_src_len, d_dst,
                       d_dst_off, d_dst_cap, d_out_len, n, attempts, (uint8_t*)d_work, slice_bytes);
    return (int)hipGetLastError();
}

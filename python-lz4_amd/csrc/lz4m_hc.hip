// lz4m_hc.hip -- hash-chain ("HC") LZ4 block compressor for MI355X (gfx950):
// lz4.block.compress(mode="high_compression"), batched.
//
// A valid LZ4 block for every input, near the size of LZ4_compress_HC at the
// same level (DESIGN.md section 9 has the measured ratios), but NOT
// byte-identical to lz4hc.c -- the contract LZ4M_PARSE_PARALLEL has towards
// LZ4_compress_default.  The parse is defined serially in DESIGN.md section 9
// and restated on the CPU by tests/hc_model/hc_model.c; this kernel produces
// that model's bytes:
//   - 13-bit hash of 4 bytes, head[h] = newest position with hash h, chain[p]
//     = distance from p to the previous position with p's hash (0: none
//     within 65535 bytes);
//   - search(q, low): up to `attempts` chain candidates below q, newest
//     first, each measured forwards from q (to n - 5) and, if >= 4 bytes
//     match, backwards (the match may start down to `low`); the longest wins,
//     the nearest among equals;
//   - parse: M = search(ip, anchor); then, while a search at M's last two
//     bytes (q = end(M) - 2, low = start(M)) finds a longer match M2, M is cut
//     at M2's start (kept if >= 4 bytes remain) and M2 takes its place.
//
// Mapping: one wavefront per block, a persistent grid striding over the
// batch.  The head table is the workgroup's LDS, cleared per block; the chain
// table is the wave's slice of the caller's workspace and is never read
// before it is written within a block, so a block's bytes do not depend on
// the wave that parsed it.
//   - Insertion runs ahead of the parse, 64 consecutive positions per step;
//     lanes that share a hash are linked by ballots over the hash bits (no
//     atomics, no reliance on the order in which one instruction's lanes
//     reach the LDS).  Position q's own chain entry is then what head[h(q)]
//     held before q went in, so a search starts from chain[q] and never sees
//     a position >= q, however far insertion has run ahead.
//   - Where no match is pending, 64 positions walk their own chains at once,
//     comparing four bytes per candidate, and the parse jumps to the first
//     position at which a search will find a match.
//   - A search gathers up to 64 chain candidates (one dependent 2-byte load
//     each, the address uniform), then every lane measures its own candidate
//     and a wave maximum picks the winner: the memory round trips of the
//     comparisons are paid once per 64 candidates.
// The kernel is bound by the latency of these dependent loads, so what counts
// is the number of resident waves, which the head table decides (HcCfg).
// The tables' constants and configurations, the insertion step and the
// sequence writer are lz4m_chain.h's, shared with lz4m_opt.hip.
//
// lz4m_compress_hc_dict_batch (hc_prefix_kernel) is the same parse for a block
// with up to 64 KiB of history lying before it in memory (a dictionary's tail,
// or the input before a linked frame's block): DESIGN.md section 9.5,
// hc_model_compress_prefix there.  Positions then count from the start of
// that prefix, which is inserted before the first search; the per-block body
// (hc_block) is shared by both entry points.
#include "lz4m_chain.h"

#include "../../include/lz4m.h"

namespace lz4m {
namespace {

constexpr int32_t kHcPrefixMax = 65536;     // history bytes used in front of a block
constexpr int32_t kHcRebasedMax = 131072;   // longest prefix + block of kHcRebased
// both kernels' slices fill the same workspace (they run one after the other)
constexpr size_t kHcWorkMax = (size_t)HcCfg<false>::kWaves * HcCfg<false>::kChain * sizeof(uint16_t);
static_assert(kHcWorkMax == (size_t)HcCfg<true>::kWaves * HcCfg<true>::kChain * sizeof(uint16_t), "shared workspace");

// The parse state of one block.  Everything is uniform across the wave.
template <int M>
struct HcBlock {
    typedef __attribute__((address_space(3))) typename HcCfg<M>::head_t head_t;
    static constexpr uint32_t kMask = HcCfg<M>::kChain - 1u;

    head_t* head;
    uint16_t* chain;
    const uint8_t* src;
    int32_t n;
    int32_t ilimit;     // positions below it can be inserted (n - 11: each has 4 bytes and may start a match)
    int32_t inserted;   // positions below it are in the tables
    int32_t attempts;
    uint32_t lane;

    // Insert 64 positions per step (hc_insert_step) until position q is in.
    __device__ __forceinline__ void insert_through(int32_t q) {
        while (inserted <= q) {
            const int32_t end = inserted + kWave < ilimit ? inserted + kWave : ilimit;
            hc_insert_step<M == kHcRebased, kMask>(head, chain, src, inserted, end, lane);
            inserted = end;
        }
    }

    // The first position >= ip (and <= mflimit) at which search() finds a
    // match, or mflimit + 1.  search(p, .) finds one exactly when one of p's
    // first `attempts` chain candidates has p's four bytes (a search position
    // has >= 7 bytes to match), so 64 positions walk their own chains at
    // once, a step per candidate, until the lowest position with such a
    // candidate has no undecided position below it.
    __device__ __forceinline__ int32_t next_candidate(int32_t ip, int32_t mflimit) {
        while (ip <= mflimit) {
            const int32_t last = ip + kWave - 1 < mflimit ? ip + kWave - 1 : mflimit;
            insert_through(last);
            const int32_t p = ip + (int32_t)lane;
            uint32_t cur = 0, want = 0;   // cur: candidate position + 1, 0 = none
            if (p <= last) {
                const uint32_t d = hc_ld(chain + ((uint32_t)p & kMask));
                cur = d ? (uint32_t)p + 1u - d : 0u;
                want = ld32(src + p);
            }
            // (a candidate lies below p and within the window by construction; checked all the same)
            bool open = cur != 0 && cur <= (uint32_t)p, hit = false;
            for (int32_t left = attempts; left > 0; --left) {
                if (open) {
                    const uint32_t c = cur - 1u;
                    const uint32_t got = ld32(src + c);
                    const uint32_t d = hc_ld(chain + (c & kMask));
                    if (got == want) {
                        hit = true;
                        open = false;
                    } else {
                        cur = d ? cur - d : 0u;
                        open = cur != 0 && cur <= (uint32_t)p && p - (int32_t)(cur - 1u) <= kHcMaxDist;
                    }
                }
                const uint64_t hits = __ballot(hit), opens = __ballot(open);
                const int fh = hits ? __builtin_ctzll(hits) : kWave, fo = opens ? __builtin_ctzll(opens) : kWave;
                if (fh < fo) return ip + fh;   // every position below it is decided: no match there
                if (opens == 0) break;
            }
            // a position still open after `attempts` candidates has none; so has every position below a late hit
            const uint64_t hits = __ballot(hit);
            if (hits) return ip + (int32_t)__builtin_ctzll(hits);
            ip = last + 1;
        }
        return ip;
    }
};

// equal bytes going backwards from a[-1] and b[-1], at most lim; reads stay at or above a - lim and b - lim
__device__ __forceinline__ int32_t hc_count_back(const uint8_t* a, const uint8_t* b, int32_t lim) {
    int32_t k = 0;
    while (k + 8 <= lim) {
        const uint64_t x = ld64(a - k - 8) ^ ld64(b - k - 8);
        if (x) return k + (int32_t)(__builtin_clzll(x) >> 3);
        k += 8;
    }
    while (k < lim && a[-k - 1] == b[-k - 1]) ++k;
    return k;
}

struct HcMatch {
    int32_t len, start, pos;   // len 0: none
};

// search(q, low); q is inserted.  All values uniform.
template <int M>
__device__ __forceinline__ HcMatch hc_search(HcBlock<M>& s, int32_t q, int32_t low) {
    constexpr uint32_t kMask = HcBlock<M>::kMask;
    const uint8_t* src = s.src;
    const int32_t lim = s.n - 5 - q;
    HcMatch m{0, 0, 0};
    // q's own entry: the newest position below q with its hash (position + 1, 0 = none)
    uint32_t cur = uni(hc_ld(s.chain + ((uint32_t)q & kMask)));
    cur = cur ? (uint32_t)q + 1u - cur : 0u;
    int32_t left = s.attempts;
    while (left > 0 && cur != 0 && q - (int32_t)(cur - 1u) <= kHcMaxDist) {
        // one lane's worth of the chain per candidate, newest in lane 0
        const int32_t take = left < kWave ? left : kWave;
        int32_t cnt = 0, mine = -1;
        do {
            if ((int32_t)s.lane == cnt) mine = (int32_t)(cur - 1u);
            ++cnt;
            const uint32_t d = uni(hc_ld(s.chain + ((cur - 1u) & kMask)));
            cur = d ? cur - d : 0u;
        } while (cnt < take && cur != 0 && q - (int32_t)(cur - 1u) <= kHcMaxDist);
        left -= cnt;
        int32_t tot = 0, back = 0;
        if (mine >= 0 && mine < q) {
            const int32_t fwd = hc_count(src + mine, src + q, lim);
            if (fwd >= 4) {
                back = hc_count_back(src + q, src + mine, q - low < mine ? q - low : mine);
                tot = fwd + back;
            }
        }
        const int32_t best = wave_max(tot);
        if (best > m.len) {
            const int l = __builtin_ctzll(__ballot(tot == best));   // the nearest of the longest
            const int32_t bk = rdl(back, l);
            m.len = best;
            m.start = q - bk;
            m.pos = rdl(mine, l) - bk;
            if (best == lim + q - low) break;   // nothing longer exists
        }
    }
    return m;
}

// One block, parsed by one wave: the n bytes at base + P, whose history is the
// P bytes before them (P = 0: section 9.1).  Positions
// count from `base`, so the block is [P, P + n); the prefix is inserted ahead
// of the first search like any other position below it, matches may start in
// it, and no emitted sequence does (anchor >= P).  Returns the block's size,
// or 0 if it does not fit in cap.  s.head, s.chain, s.attempts and s.lane are
// set by the caller.
template <int M>
__device__ __forceinline__ int32_t hc_block(HcBlock<M>& s, const uint8_t* base, int32_t P, int32_t n, uint8_t* dst,
                                            int32_t cap) {
    const uint32_t lane = s.lane;
    const int32_t total = P + n;
    int32_t op = 0, anchor = P;
    bool fits = true;
    if (n >= 13) {
        for (int32_t i = (int32_t)lane; i < kHcHeads; i += kWave) hc_st(s.head + i, 0u);
        hc_fence();
        const int32_t mflimit = total - 12;
        s.src = base;
        s.n = total;
        s.ilimit = mflimit + 1;
        s.inserted = 0;
        if (P > 0) s.insert_through(P - 1);
        int32_t ip = P;
        while ((ip = s.next_candidate(ip, mflimit)) <= mflimit) {
            HcMatch m = hc_search(s, ip, anchor);
            if (m.len == 0) {
                ++ip;
                continue;
            }
            for (;;) {   // probe the end of the match for a longer one that overlaps it
                const int32_t q = m.start + m.len - 2;
                if (q > mflimit) break;
                s.insert_through(q);
                const HcMatch m2 = hc_search(s, q, m.start);
                if (m2.len <= m.len) break;
                if (m2.start - m.start >= 4) {   // keep the head of the first match
                    fits = hc_emit(dst, op, cap, base, anchor, m.start - anchor, m.start - m.pos,
                                   m2.start - m.start, lane);
                    if (!fits) break;
                    anchor = m2.start;
                }
                m = m2;
            }
            if (fits) fits = hc_emit(dst, op, cap, base, anchor, m.start - anchor, m.start - m.pos, m.len, lane);
            if (!fits) break;
            ip = m.start + m.len;
            anchor = ip;
        }
    }
    if (fits) fits = hc_emit(dst, op, cap, base, anchor, total - anchor, 0, 0, lane);
    return fits ? op : 0;
}

// The persistent grid of both entry points: wave blockIdx.x takes every
// gridDim.x-th block of the batch.  dict_len == nullptr (known at compile time
// in hc_compress_kernel): no block has a prefix.  Configuration kHcSmall takes
// the blocks whose prefix + length is at most kHcSmallMax bytes, kHcRebased
// (with a prefix only) those up to kHcRebasedMax, kHcBig the others.
template <int M, bool PREFIX>
__device__ __forceinline__ void hc_grid(const uint8_t* __restrict__ src_base, const int64_t* __restrict__ src_off,
                                        const int32_t* __restrict__ src_len, const int32_t* __restrict__ dict_len,
                                        uint8_t* __restrict__ dst_base, const int64_t* __restrict__ dst_off,
                                        const int32_t* __restrict__ dst_cap, int32_t* __restrict__ out_len,
                                        int64_t nblocks, int32_t attempts, uint16_t* __restrict__ work) {
    typedef typename HcCfg<M>::head_t head_mem_t;
    __shared__ __attribute__((aligned(16))) head_mem_t head_mem[kHcHeads];
    HcBlock<M> s;
    s.head = (typename HcBlock<M>::head_t*)head_mem;
    s.chain = work + (size_t)blockIdx.x * HcCfg<M>::kChain;
    s.attempts = attempts;
    s.lane = threadIdx.x;
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int32_t n = src_len[b];
        int32_t P = 0;
        if (PREFIX) {
            const int32_t dl = dict_len[b];
            P = dl < 0 ? 0 : (dl < kHcPrefixMax ? dl : kHcPrefixMax);
        }
        // (a negative n is refused below by either kernel; the small one takes it)
        const int64_t total = (int64_t)P + (n < 0 ? 0 : n);
        const int mine = total <= kHcSmallMax ? kHcSmall : (PREFIX && total <= kHcRebasedMax ? kHcRebased : kHcBig);
        if (mine != M) continue;   // another kernel's block
        const int32_t cap = dst_cap[b];
        if (n < 0 || n > kHcMaxInput || cap < 0) {
            if (s.lane == 0) out_len[b] = 0;
            continue;
        }
        const int32_t r = hc_block<M>(s, src_base + src_off[b] - P, P, n, dst_base + dst_off[b], cap);
        if (s.lane == 0) out_len[b] = r;
    }
}

// lz4m_compress_hc_batch's kernels (no prefix)
template <bool BIG>
__global__ __launch_bounds__(64) void hc_compress_kernel(const uint8_t* __restrict__ src_base,
                                                         const int64_t* __restrict__ src_off,
                                                         const int32_t* __restrict__ src_len,
                                                         uint8_t* __restrict__ dst_base,
                                                         const int64_t* __restrict__ dst_off,
                                                         const int32_t* __restrict__ dst_cap,
                                                         int32_t* __restrict__ out_len, int64_t nblocks,
                                                         int32_t attempts, uint16_t* __restrict__ work) {
    hc_grid<BIG ? kHcBig : kHcSmall, false>(src_base, src_off, src_len, nullptr, dst_base, dst_off, dst_cap, out_len, nblocks, attempts,
                                            work);
}

// lz4m_compress_hc_dict_batch's kernels: block b's history is the last
// min(dict_len[b], 65536) bytes before it in src
template <int M>
__global__ __launch_bounds__(64) void hc_prefix_kernel(const uint8_t* __restrict__ src_base,
                                                       const int64_t* __restrict__ src_off,
                                                       const int32_t* __restrict__ src_len,
                                                       const int32_t* __restrict__ dict_len,
                                                       uint8_t* __restrict__ dst_base,
                                                       const int64_t* __restrict__ dst_off,
                                                       const int32_t* __restrict__ dst_cap,
                                                       int32_t* __restrict__ out_len, int64_t nblocks,
                                                       int32_t attempts, uint16_t* __restrict__ work) {
    hc_grid<M, true>(src_base, src_off, src_len, dict_len, dst_base, dst_off, dst_cap, out_len, nblocks, attempts,
                     work);
}

}  // namespace
}  // namespace lz4m

extern "C" size_t lz4m_compress_hc_workspace_size(int64_t n, int32_t max_len) {
    using namespace lz4m;
    if (n <= 0 || max_len < 0) return 0;
    // the longer blocks' kernel has half the waves with slices twice as large
    const int64_t waves = n < HcCfg<false>::kWaves ? n : HcCfg<false>::kWaves;
    const size_t bytes = (size_t)waves * HcCfg<true>::kChain * sizeof(uint16_t);
    return bytes < kHcWorkMax ? bytes : kHcWorkMax;
}

extern "C" size_t lz4m_compress_hc_dict_workspace_size(int64_t n, int32_t max_len) {
    using namespace lz4m;
    if (n <= 0 || max_len < 0) return 0;
    // a 256 KiB slice for every wave of the widest grid (kHcRebased)
    const int64_t waves = n < HcCfg<kHcRebased>::kWaves ? n : HcCfg<kHcRebased>::kWaves;
    return (size_t)waves * HcCfg<kHcRebased>::kChain * sizeof(uint16_t);
}

extern "C" int lz4m_compress_hc_batch(const uint8_t* d_src, const int64_t* d_src_off, const int32_t* d_src_len,
                                      uint8_t* d_dst, const int64_t* d_dst_off, const int32_t* d_dst_cap,
                                      int32_t* d_out_len, int64_t n, int level, void* d_work, size_t work_bytes,
                                      lz4m_stream_t stream) {
    using namespace lz4m;
    if (n < 0) return LZ4M_EINVAL;
    if (n == 0) return 0;
    if (d_work == nullptr || ((uintptr_t)d_work & 1u) || work_bytes < lz4m_compress_hc_workspace_size(n, 0))
        return LZ4M_EINVAL;
    const int32_t attempts = hc_attempts(level);
    hipStream_t st = (hipStream_t)stream;
    // both kernels walk the whole batch and take their own blocks; a wave
    // whose share holds none of them ends after reading its blocks' lengths
    const uint32_t small_grid = (uint32_t)(n < HcCfg<false>::kWaves ? n : HcCfg<false>::kWaves);
    hipLaunchKernelGGL(hc_compress_kernel<false>, dim3(small_grid), dim3(64), 0, st, d_src, d_src_off, d_src_len,
                       d_dst, d_dst_off, d_dst_cap, d_out_len, n, attempts, (uint16_t*)d_work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const uint32_t big_grid = (uint32_t)(n < HcCfg<true>::kWaves ? n : HcCfg<true>::kWaves);
    hipLaunchKernelGGL(hc_compress_kernel<true>, dim3(big_grid), dim3(64), 0, st, d_src, d_src_off, d_src_len,
                       d_dst, d_dst_off, d_dst_cap, d_out_len, n, attempts, (uint16_t*)d_work);
    return (int)hipGetLastError();
}

extern "C" int lz4m_compress_hc_dict_batch(const uint8_t* d_src, const int64_t* d_src_off, const int32_t* d_src_len,
                                           const int32_t* d_dict_len, uint8_t* d_dst, const int64_t* d_dst_off,
                                           const int32_t* d_dst_cap, int32_t* d_out_len, int64_t n, int level,
                                           void* d_work, size_t work_bytes, lz4m_stream_t stream) {
    using namespace lz4m;
    if (n < 0) return LZ4M_EINVAL;
    if (n == 0) return 0;
    if (d_dict_len == nullptr || d_work == nullptr || ((uintptr_t)d_work & 1u) ||
        work_bytes < lz4m_compress_hc_workspace_size(n, 0))
        return LZ4M_EINVAL;
    const int32_t attempts = hc_attempts(level);
    hipStream_t st = (hipStream_t)stream;
    // as above, one launch per configuration: prefix + length <= 64 KiB, <= 128 KiB, longer
    const uint32_t small_grid = (uint32_t)(n < HcCfg<kHcSmall>::kWaves ? n : HcCfg<kHcSmall>::kWaves);
    hipLaunchKernelGGL(hc_prefix_kernel<kHcSmall>, dim3(small_grid), dim3(64), 0, st, d_src, d_src_off, d_src_len,
                       d_dict_len, d_dst, d_dst_off, d_dst_cap, d_out_len, n, attempts, (uint16_t*)d_work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    // (a wave per 256 KiB slice the workspace holds: at least kHcBig's grid, twice that with
    // lz4m_compress_hc_dict_workspace_size bytes)
    int64_t slices = (int64_t)(work_bytes / (HcCfg<kHcRebased>::kChain * sizeof(uint16_t)));
    if (slices > HcCfg<kHcRebased>::kWaves) slices = HcCfg<kHcRebased>::kWaves;
    const uint32_t mid_grid = (uint32_t)(n < slices ? n : slices);
    hipLaunchKernelGGL(hc_prefix_kernel<kHcRebased>, dim3(mid_grid), dim3(64), 0, st, d_src, d_src_off, d_src_len,
                       d_dict_len, d_dst, d_dst_off, d_dst_cap, d_out_len, n, attempts, (uint16_t*)d_work);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const uint32_t big_grid = (uint32_t)(n < HcCfg<kHcBig>::kWaves ? n : HcCfg<kHcBig>::kWaves);
    hipLaunchKernelGGL(hc_prefix_kernel<kHcBig>, dim3(big_grid), dim3(64), 0, st, d_src, d_src_off, d_src_len,
                       d_dict_len, d_dst, d_dst_off, d_dst_cap, d_out_len, n, attempts, (uint16_t*)d_work);
    return (int)hipGetLastError();
}

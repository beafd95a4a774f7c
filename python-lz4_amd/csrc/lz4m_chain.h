// lz4m_chain.h -- what the hash-chain parses share (lz4m_hc.hip: HC, without
// and with a prefix; lz4m_opt.hip: optimal): the tables of DESIGN.md section
// 9.1 (a 13-bit hash of 4 bytes, head[h] = newest position with hash h, plus
// 1; chain[p] = distance from p to the previous position with p's hash, 0:
// none within 65535 bytes), their configurations, the lz4hc level table, the
// insertion step and the sequence writer.  tests/hc_model/hc_model.c is the
// same on the CPU.  Included by those two translation units only.
#pragma once

#include "lz4m_common.h"

namespace lz4m {

constexpr int kHcHashBits = 13;
constexpr int kHcHeads = 1 << kHcHashBits;
constexpr int32_t kHcMaxDist = 65535;    // LZ4_DISTANCE_MAX
constexpr int32_t kHcSmallMax = 65536;   // longest prefix + block of kHcSmall (u16 heads hold position + 1)
constexpr int32_t kHcMaxInput = 0x7E000000;

// Three configurations share the tables (M; false / true name the first two).
// kHcSmall: blocks of up to 64 KiB, prefix included: u16 heads (position + 1
// <= 65525; 16 KiB of LDS, 10 workgroups per CU of 160 KiB) and a chain
// indexed by the position.  kHcBig: u32 heads (32 KiB, 5 per CU) and a chain
// of 2 x 65536 entries indexed by the position mod 131072: positions are
// inserted up to 127 ahead of a search, and a window of exactly 65536 entries
// would overwrite that search's oldest candidates.  kHcRebased (prefix kernel
// only): prefix + block of 65537..131072 bytes, the 64 KiB block of a linked
// frame; u16 heads again, holding (position mod 65535) + 1, with kHcBig's
// chain.  Such an entry names the positions d, d + 65535, ... back (d in
// 1..65535), of which only the first is within LZ4_DISTANCE_MAX; it is the
// newest position with the hash exactly when its four bytes hash to it (a
// nearer position with that hash would have replaced the entry), which
// insertion checks, so the chain is the one kHcBig builds.  (The optimal
// parse keeps a chain entry per position of its block and uses head_t and
// kWaves alone.)
constexpr int kHcSmall = 0, kHcBig = 1, kHcRebased = 2;
template <int M>
struct HcCfg {
    typedef uint16_t head_t;
    static constexpr int kWaves = 2560;
    static constexpr uint32_t kChain = 65536;
};
template <>
struct HcCfg<kHcBig> {
    typedef uint32_t head_t;
    static constexpr int kWaves = 1280;
    static constexpr uint32_t kChain = 131072;
};
template <>
struct HcCfg<kHcRebased> {
    typedef uint16_t head_t;
    static constexpr int kWaves = 2560;   // as many of them as the caller's workspace has slices for
    static constexpr uint32_t kChain = 131072;
};

// lz4hc.c level table: levels below 1 mean 9; 1-2 -> 2 attempts, 3 -> 4, ...
// 9 -> 256; deeper searches for levels 10-12 are not built (HC searches as 9
// there, and so does the optimal parse, the higher-ratio one of the two)
inline int32_t hc_attempts(int level) {
    if (level < 1) level = 9;
    if (level > 9) level = 9;
    return level < 3 ? 2 : 1 << (level - 1);
}

// One step of hash-chain insertion takes 64 consecutive positions, lane l the
// l-th (act: it is inserted, h: its hash of BITS bits).  The lanes that share
// a hash are found by ballots over the hash bits (no atomics, no reliance on
// the order in which one instruction's lanes reach the LDS): `below` / `above`
// are the active lanes under / over this one with its hash.  A position chains
// to the highest lane of `below`, else to the table's entry; the lane with no
// `above` writes the table.
template <int BITS>
__device__ __forceinline__ void hash_links(bool act, uint32_t h, uint32_t lane, uint64_t& below, uint64_t& above) {
    uint64_t same = __ballot(act);
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const bool bit = (h >> b) & 1u;
        const uint64_t B = __ballot(bit);
        same &= bit ? B : ~B;
    }
    below = same & ((1ull << lane) - 1ull);
    above = same & ~((2ull << lane) - 1ull);
}

// accesses of one lane that another lane of the wave made or will make:
// relaxed atomics at wavefront scope (plain loads and stores in the ISA),
// ordered by hc_fence
template <typename T>
__device__ __forceinline__ uint32_t hc_ld(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
template <typename T>
__device__ __forceinline__ void hc_st(T* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ void hc_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// equal leading bytes of a[..] and b[..], at most lim; reads stay below a + lim and b + lim
__device__ __forceinline__ int32_t hc_count(const uint8_t* a, const uint8_t* b, int32_t lim) {
    int32_t k = 0;
    while (k + 8 <= lim) {
        const uint64_t x = ld64(a + k) ^ ld64(b + k);
        if (x) return k + (int32_t)(__builtin_ctzll(x) >> 3);
        k += 8;
    }
    while (k < lim && a[k] == b[k]) ++k;
    return k;
}

// the e = ext_len<true>(v) length bytes of v at o
__device__ __forceinline__ void hc_put_ext(uint8_t* o, int32_t v, int32_t e, uint32_t lane) {
    if (e == 0) return;
    for (int32_t k = (int32_t)lane; k < e - 1; k += kWave) o[k] = 255;
    if (lane == 0) o[e - 1] = (uint8_t)(v - 15 - 255 * (e - 1));
}

// One sequence at dst + op: ll literals from src + anchor, then (ml > 0) a
// match of ml bytes at distance off; ml == 0 is the block's last sequence.
// False (nothing written) if it does not fit in cap.
__device__ __forceinline__ bool hc_emit(uint8_t* dst, int32_t& op, int32_t cap, const uint8_t* src, int32_t anchor,
                                        int32_t ll, int32_t off, int32_t ml, uint32_t lane) {
    const int32_t le = ext_len<true>(ll), me = ml ? ext_len<true>(ml - 4) : 0;
    const int64_t need = 1 + (int64_t)le + ll + (ml ? 2 + me : 0);
    if ((int64_t)op + need > (int64_t)cap) return false;
    uint8_t* o = dst + op;
    if (lane == 0) {
        const int32_t mt = ml ? (ml - 4 < 15 ? ml - 4 : 15) : 0;
        o[0] = (uint8_t)(((ll < 15 ? ll : 15) << 4) | mt);
    }
    hc_put_ext(o + 1, ll, le, lane);
    uint8_t* lit = o + 1 + le;
    for (int32_t k = (int32_t)lane; k < ll; k += kWave) lit[k] = src[anchor + k];
    if (ml) {
        uint8_t* mo = lit + ll;
        if (lane == 0) {
            mo[0] = (uint8_t)(off & 0xFF);
            mo[1] = (uint8_t)(off >> 8);
        }
        hc_put_ext(mo + 2, ml - 4, me, lane);
    }
    op += (int32_t)need;
    return true;
}

// kHcRebased: position (< 131072) mod 65535
__device__ __forceinline__ uint32_t hc_rebased(uint32_t p) {
    return p >= 131070u ? p - 131070u : (p >= 65535u ? p - 65535u : p);
}

// One insertion step: the positions [base, min(base + 64, end)), lane l the
// l-th.  A position chains to the nearest earlier lane of the step with the
// same hash, else to the table's entry; the last lane of each hash writes the
// table.  REBASED: the heads are kHcRebased's; MASK: the chain is indexed by
// the position & MASK (kNoMask: by the position itself).
constexpr uint32_t kNoMask = 0xFFFFFFFFu;
template <bool REBASED, uint32_t MASK, typename HEAD>
__device__ __forceinline__ void hc_insert_step(HEAD* head, uint16_t* chain, const uint8_t* src, int32_t base,
                                               int32_t end, uint32_t lane) {
    const int32_t p = base + (int32_t)lane;
    const bool act = p < end;
    uint32_t h = 0;
    if (act) h = hash4<kHcHashBits>(ld32(src + p));
    uint64_t below, above;
    hash_links<kHcHashBits>(act, h, lane, below, above);
    if (act) {
        uint32_t prev = below ? (uint32_t)base + (63u - (uint32_t)__builtin_clzll(below)) + 1u : hc_ld(head + h);
        if (REBASED && !below && prev) {
            const uint32_t r = hc_rebased((uint32_t)p), e = prev - 1u;
            const uint32_t back = r > e ? r - e : r + 65535u - e;   // 1..65535
            prev = back <= (uint32_t)p && hash4<kHcHashBits>(ld32(src + p - (int32_t)back)) == h
                       ? (uint32_t)p + 1u - back
                       : 0u;
        }
        const uint32_t d = prev ? (uint32_t)p + 1u - prev : 0u;
        hc_st(MASK == kNoMask ? chain + p : chain + ((uint32_t)p & MASK), d > (uint32_t)kHcMaxDist ? 0u : d);
        if (above == 0) hc_st(head + h, REBASED ? hc_rebased((uint32_t)p) + 1u : (uint32_t)p + 1u);
    }
    hc_fence();
}

}  // namespace lz4m

// lz4m_common.h -- shared device helpers for the MI355X LZ4 kernels (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lz4m {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// a byte in LDS (address space 3): LDS and HBM accesses stay distinct
// instructions (ds_* vs global_*), never merged into generic flat accesses,
// which the compiler must fence with vmcnt(0) + lgkmcnt(0)
typedef __attribute__((address_space(3))) uint8_t lds_u8;
__device__ __forceinline__ u32x4 lds_ld16(const lds_u8* p) {
    u32x4 v;
    __builtin_memcpy(&v, (const uint8_t*)p, 16);
    return v;
}
__device__ __forceinline__ void lds_st16(lds_u8* p, u32x4 v) { __builtin_memcpy((uint8_t*)p, &v, 16); }

constexpr int kWave = 64;

// 16-byte accesses at any byte alignment: gfx950 runs in unaligned-access
// mode, so these lower to one global_load/store_dwordx4.
__device__ __forceinline__ u32x4 ld16(const uint8_t* p) {
    u32x4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
__device__ __forceinline__ void st16(uint8_t* p, u32x4 v) { __builtin_memcpy(p, &v, 16); }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint64_t ld64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// 16 bytes at p, with bytes at or beyond `avail` read as zero (never
// touches memory past p + avail).
__device__ __forceinline__ u32x4 ld16_guarded(const uint8_t* p, int64_t avail) {
    if (avail >= 16) return ld16(p);
    uint64_t lo = 0, hi = 0;
    const int n = avail <= 0 ? 0 : (int)avail;
    for (int k = 0; k < n; ++k) {
        const uint64_t b = p[k];
        if (k < 8) lo |= b << (8 * k);
        else hi |= b << (8 * (k - 8));
    }
    return u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
}

// The 4 bytes starting at byte k (0..15) of the 16-byte window w; bytes past
// the window read as zero.
__device__ __forceinline__ uint32_t window_dword(u32x4 w, uint32_t k) {
    const uint32_t q = k >> 2;
    const uint32_t lo = q == 0 ? w.x : q == 1 ? w.y : q == 2 ? w.z : w.w;
    const uint32_t hi = q == 0 ? w.y : q == 1 ? w.z : q == 2 ? w.w : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, k & 3);
}

// Window shifted down by one byte (byte 15 reads as zero).
__device__ __forceinline__ u32x4 window_shift1(u32x4 w) {
    return u32x4{__builtin_amdgcn_alignbyte(w.y, w.x, 1), __builtin_amdgcn_alignbyte(w.z, w.y, 1),
                 __builtin_amdgcn_alignbyte(w.w, w.z, 1), __builtin_amdgcn_alignbyte(0u, w.w, 1)};
}

__device__ __forceinline__ uint32_t byte_of(u32x4 w, int k) {
    const uint32_t d = (k >> 2) == 0 ? w.x : (k >> 2) == 1 ? w.y : (k >> 2) == 2 ? w.z : w.w;
    return (d >> ((k & 3) * 8)) & 0xFFu;
}

// Expand the first `off` (1..15) bytes of w into a 16-byte pattern with
// period `off`: E[j] = w[j % off].  Doubling keeps the valid length a
// multiple of `off`.
__device__ __forceinline__ u32x4 period_pattern(u32x4 w, uint32_t off) {
    uint64_t lo = ((uint64_t)w.y << 32) | w.x;
    uint64_t hi = ((uint64_t)w.w << 32) | w.z;
    if (off < 8) {
        lo &= (1ull << (8 * off)) - 1ull;
        hi = 0;
    } else if (off == 8) {
        hi = 0;
    } else {
        hi &= (1ull << (8 * (off - 8))) - 1ull;
    }
    for (uint32_t len = off; len < 16; len *= 2) {
        const uint32_t s = 8 * len;   // 8..120, multiple of 8
        uint64_t slo, shi;
        if (s >= 64) {
            shi = lo << (s - 64);
            slo = 0;
        } else {
            shi = (hi << s) | (lo >> (64 - s));
            slo = lo << s;
        }
        lo |= slo;
        hi |= shi;
    }
    return u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
}

// ---------------------------------------------------- aligned LDS access
// A _b64 / _b128 LDS access off its natural alignment -- and a _b32 one off
// 4 bytes -- replays at ~56 cycles per wave-instruction on gfx950
// (tools/micro/lds_align.hip; cdna_hip_programming.md Guideline 17), and the
// decoders' history buffers are read and written at arbitrary byte offsets.
// So both are made of naturally aligned dword accesses only:
// - a 16-byte read at any offset is five aligned dwords (two ds_read2_b32 and
//   one ds_read_b32) and four alignbytes;
// - an exact put of k <= 16 bytes is five ds_mskor_b32 (dst = dst & ~mask |
//   data) on the enclosing aligned dwords -- atomic per dword, so
//   neighbouring sequences that share a boundary dword can be written by one
//   instruction -- with the masks from a table by (address & 3, k) and each
//   dword's bytes placed by one v_perm with a per-lane selector (0x0C, a zero
//   byte, outside the put).
typedef __attribute__((address_space(3))) volatile uint64_t lds_vu64;
typedef __attribute__((address_space(3))) const uint32_t lds_cu32;
typedef __attribute__((address_space(3))) const uint32_t lds_cu32a __attribute__((aligned(4)));
__device__ __forceinline__ uint32_t lds_addr(const lds_u8* p) { return (uint32_t)(uintptr_t)p; }
__device__ __forceinline__ u32x4 lds_ld16a(const lds_u8* p) {
    const uint32_t a = lds_addr(p), r = a & 3u;
    const lds_cu32a* q = (const lds_cu32a*)(p - r);
    const uint32_t c0 = q[0], c1 = q[1], c2 = q[2], c3 = q[3], c4 = q[4];
    return u32x4{__builtin_amdgcn_alignbyte(c1, c0, r), __builtin_amdgcn_alignbyte(c2, c1, r),
                 __builtin_amdgcn_alignbyte(c3, c2, r), __builtin_amdgcn_alignbyte(c4, c3, r)};
}
// byte masks of an exact put of k (0..16) bytes at address & 3 == r over the
// enclosing dwords 0..3: table entry (r * 17 + k), 16 bytes (dword 4 is
// computed); built once per workgroup by lds_put_table_init
constexpr int kPutTab = 4 * 17 * 4;
__device__ __forceinline__ void lds_put_table_init(uint32_t* tab, uint32_t lane, uint32_t nlanes) {
    for (uint32_t e = lane; e < (uint32_t)kPutTab; e += nlanes) {
        const uint32_t i = e & 3u, ent = e >> 2, k = ent % 17u, r = ent / 17u;
        uint32_t m = 0;
        for (uint32_t b = 0; b < 4; ++b) {
            const uint32_t pos = 4u * i + b;   // byte of the 16..20-byte span
            if (pos >= r && pos < r + k) m |= 0xFFu << (8 * b);
        }
        tab[e] = m;
    }
}
// Exactly k bytes (k >= 16: 16) of v at LDS address p.
__device__ __forceinline__ void lds_put_al(lds_u8* p, u32x4 v, int32_t k, lds_cu32* tab) {
    const uint32_t a = lds_addr(p), r = a & 3u;
    const uint32_t kk = k >= 16 ? 16u : (uint32_t)k;
    // destination dword i, byte b holds put byte 4i + b - r: v_perm of
    // (v[i], v[i-1]) with selector byte 4 + b - r, 0x0C (zero) where the
    // mask says the byte is not the put's
    u32x4 m;
    __builtin_memcpy(&m, (const uint8_t*)(tab + 4u * (r * 17u + kk)), 16);   // 16-byte aligned
    const int32_t t4 = (int32_t)(r + kk) - 16;   // bytes in dword 4 (0..3)
    const uint32_t m4 = t4 > 0 ? (1u << (8 * t4)) - 1u : 0u;
    // r replicated into every byte by one v_perm (a v_mul_lo_u32 is quarter rate)
    const uint32_t sb = 0x07060504u - __builtin_amdgcn_perm(0u, r, 0u);
    const uint32_t b4 = a & ~3u;
    auto sel = [&](uint32_t mk) __attribute__((always_inline)) { return (mk & sb) | (~mk & 0x0C0C0C0Cu); };
    const uint32_t d0 = __builtin_amdgcn_perm(v.x, v.x, sel(m.x));
    const uint32_t d1 = __builtin_amdgcn_perm(v.y, v.x, sel(m.y));
    const uint32_t d2 = __builtin_amdgcn_perm(v.z, v.y, sel(m.z));
    const uint32_t d3 = __builtin_amdgcn_perm(v.w, v.z, sel(m.w));
    const uint32_t d4 = __builtin_amdgcn_perm(0u, v.w, sel(m4));
    asm volatile("ds_mskor_b32 %0, %1, %2 offset:0" ::"v"(b4), "v"(m.x), "v"(d0) : "memory");
    asm volatile("ds_mskor_b32 %0, %1, %2 offset:4" ::"v"(b4), "v"(m.y), "v"(d1) : "memory");
    asm volatile("ds_mskor_b32 %0, %1, %2 offset:8" ::"v"(b4), "v"(m.z), "v"(d2) : "memory");
    asm volatile("ds_mskor_b32 %0, %1, %2 offset:12" ::"v"(b4), "v"(m.w), "v"(d3) : "memory");
    asm volatile("ds_mskor_b32 %0, %1, %2 offset:16" ::"v"(b4), "v"(m4), "v"(d4) : "memory");
}

// ------------------------------------------------ period-pattern selectors
// A match with offset off < 16 repeats its first off bytes: output byte j is
// w[j % off] (LZ4_memcpy_using_offset, lz4.c:513-551).  Selector table: 8
// dwords per offset (16 x 8 = 128), entry (off, i) builds output dword i >> 1
// from bytes 0-7 (i even) or 8-15 (i odd) of w; 0x0C selects a zero byte.
__device__ __forceinline__ void period_sel_init(uint32_t* psel, uint32_t tid, uint32_t nthreads) {
    for (uint32_t e = tid; e < 16u * 8u; e += nthreads) {
        const uint32_t o = e >> 3, i = e & 7, hi = i & 1;
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4; ++b) {
            const uint32_t x = o ? (4 * (i >> 1) + b) % o : 0;
            const uint32_t sb = hi ? (x >= 8 ? x - 8 : 0x0C) : (x < 8 ? x : 0x0C);
            v |= sb << (8 * b);
        }
        psel[e] = v;
    }
}
// Period-off pattern of the first off (1..15) bytes of w, E[j] = w[j % off]:
// per output dword, v_perm from bytes 0-7 and from bytes 8-15 with the
// selectors sel = psel + 8 * off.
__device__ __forceinline__ u32x4 period_perm(u32x4 w, lds_cu32* sel) {
    u32x4 r;
    r.x = __builtin_amdgcn_perm(w.y, w.x, sel[0]) | __builtin_amdgcn_perm(w.w, w.z, sel[1]);
    r.y = __builtin_amdgcn_perm(w.y, w.x, sel[2]) | __builtin_amdgcn_perm(w.w, w.z, sel[3]);
    r.z = __builtin_amdgcn_perm(w.y, w.x, sel[4]) | __builtin_amdgcn_perm(w.w, w.z, sel[5]);
    r.w = __builtin_amdgcn_perm(w.y, w.x, sel[6]) | __builtin_amdgcn_perm(w.w, w.z, sel[7]);
    return r;
}

// -------------------------------------------------------- lane broadcast
__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

__device__ __forceinline__ int64_t readlane64(int64_t v, int lane) {
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), lane);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
// A lane's global-memory pointer, broadcast.  Rebuilt as a global
// (address space 1) pointer, so accesses through it stay global_* (not flat).
template <typename T>
__device__ __forceinline__ T* readlane_ptr(T* p, int lane) {
    typedef __attribute__((address_space(1))) T gT;
    gT* g = (gT*)(uintptr_t)readlane64(reinterpret_cast<int64_t>(p), lane);
    return (T*)g;
}
// lane l's v / the first active lane's v, as a uniform value
__device__ __forceinline__ int32_t rdl(int32_t v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// ------------------------------------------------------------- DPP scans
// Inclusive prefix scans, VALU only.  A row = 16 consecutive lanes: row_shr
// 1/2/4/8 stays inside a row; row_bcast:15 / row_bcast:31 then carry the row
// totals across the wave.
__device__ __forceinline__ int32_t row_incl_sum(int32_t v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);   // row_shr:8
    return v;
}
__device__ __forceinline__ int32_t wave_incl_sum(int32_t v) {
    v = row_incl_sum(v);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);   // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);   // row_bcast:31 -> rows 2, 3
    return v;
}
// prefix maximum (v >= 0: the identity is 0), the same steps
__device__ __forceinline__ int32_t row_incl_max(int32_t v) {
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false));
    return v;
}
__device__ __forceinline__ int32_t wave_incl_max(int32_t v) {
    v = row_incl_max(v);
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false));
    return v;
}
// the wave's largest v (v >= 0), uniform
__device__ __forceinline__ int32_t wave_max(int32_t v) { return rdl(wave_incl_max(v), 63); }

// ------------------------------------------------------ LZ4 block format
// hash of 4 bytes into BITS bits (LZ4_hash4, lz4.c:756-762)
template <int BITS>
__device__ __forceinline__ uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - BITS); }

// y / 255 for y >= 0.  Blocks <= 64 KiB (!BIG): (z + z/256) / 256 with z =
// y + 1, exact for y < 65 790 (checked exhaustively), two shifts and two adds
// where the division is a quarter-rate v_mul_hi_u32
template <bool BIG>
__device__ __forceinline__ int32_t div255(int32_t y) {
    if (BIG) return y / 255;
    const int32_t z = y + 1;
    return (z + (z >> 8)) >> 8;
}
// length bytes after the token for a length field x (0 below 15)
template <bool BIG>
__device__ __forceinline__ int32_t ext_len(int32_t x) { return x >= 15 ? 1 + div255<BIG>(x - 15) : 0; }

// read_variable_length (lz4.c:1903-1928) over a stream read 16 bytes at a
// time: in16(p) = the 16 stream bytes at p, with bytes at or beyond the
// block's end read as zero.  On failure ip is the position the reference
// reports.
template <typename In16>
__device__ __forceinline__ bool len_run(In16&& in16, int64_t& ip, int64_t ilimit, bool initial_check, int64_t& out) {
    if (initial_check && ip >= ilimit) return false;
    // 16 bytes per load: a run of 255s (a long literal or match, e.g. the
    // 257 length bytes of a stored-looking 64 KiB block) costs one memory
    // round trip per 16 bytes instead of per byte.  Same outcome as the
    // reference's byte loop: reading the byte at ilimit fails with
    // ip = ilimit + 1 (ilimit < iend, so every byte up to it is readable;
    // in16 zero-fills past iend, i.e. past ilimit).
    if (ip >= ilimit) {   // the first byte read already fails (ip + 1)
        ++ip;
        return false;
    }
    int64_t len = 0;
    for (;;) {
        const u32x4 v = in16(ip);
        const uint32_t n0 = ~v.x, n1 = ~v.y, n2 = ~v.z, n3 = ~v.w;
        const uint32_t q = n0 ? 0u : n1 ? 1u : n2 ? 2u : n3 ? 3u : 4u;
        if (q < 4) {
            const uint32_t nw = q == 0 ? n0 : q == 1 ? n1 : q == 2 ? n2 : n3;
            const uint32_t bi = (uint32_t)__builtin_ctz(nw) >> 3;
            const uint32_t j = 4 * q + bi;   // first byte != 255
            if (ip + (int64_t)j >= ilimit) {
                ip = ilimit + 1;
                return false;
            }
            len += 255 * (int64_t)j + (int64_t)((~nw >> (8 * bi)) & 0xFFu);   // no indexed access: no scratch
            ip += j + 1;
            out = len;
            return true;
        }
        if (ip + 16 > ilimit) {   // the run reaches ilimit
            ip = ilimit + 1;
            return false;
        }
        len += 255 * 16;
        ip += 16;
    }
}

// ------------------------------------------------------------ exact puts
// Store exactly k (0..16) bytes of v at global address p (any alignment).
__device__ __forceinline__ void put_exact(uint8_t* p, u32x4 v, uint32_t k) {
    if (k == 16) {
        st16(p, v);
        return;
    }
    uint32_t o = 0;
    if (k & 8) {
        const uint64_t x = ((uint64_t)v.y << 32) | v.x;
        __builtin_memcpy(p, &x, 8);
        o = 8;
    }
    if (k & 4) {
        const uint32_t x = window_dword(v, o);
        __builtin_memcpy(p + o, &x, 4);
        o += 4;
    }
    if (k & 2) {
        const uint16_t x = (uint16_t)window_dword(v, o);
        __builtin_memcpy(p + o, &x, 2);
        o += 2;
    }
    if (k & 1) p[o] = (uint8_t)window_dword(v, o);
}
// The same for any k: nothing for k <= 0, 16 bytes for k >= 16 (k = the
// bytes left of a copy taken in 16-byte pieces).
__device__ __forceinline__ void gbl_put(uint8_t* p, u32x4 v, int32_t k) {
    if (k >= 16) {
        st16(p, v);
    } else if (k > 0) {
        put_exact(p, v, (uint32_t)k);
    }
}

// -------------------------------------------------------- wild wave copy
// Non-overlapping copy of len bytes by the whole wave (uniform arguments).
// Wild: the tail may be written as a whole 16-byte piece where d_room and
// s_room (the bytes of the block's own buffers from d / s on) allow it, like
// the reference's wild copies; it never writes past d + d_room or reads past
// s + s_room.  Each lane requests kU 16-byte pieces before storing any: a long
// literal (a stored-looking block's 64 KiB) waits on one memory round trip
// per 4 KiB instead of per 1 KiB (kU = 1 where registers are short: the
// dictionary kernel).
// SL: s points into LDS (the lone-block decoder's staged input): LDS reads,
// which wait on no store, where a flat read of LDS waits for every store the
// wave has in flight (one L2 write round trip per 4 KiB of a long literal).
template <int kU = 4, bool SL = false>
__device__ __forceinline__ void wave_copy_wild(uint8_t* d, const uint8_t* s, int64_t len, int64_t d_room,
                                               int64_t s_room, uint32_t lane) {
    for (int64_t base = 0; base < len; base += 16 * kWave * kU) {
        u32x4 v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t pos = base + 16 * kWave * u + 16 * (int64_t)lane;
            const bool whole = pos < len && (len - pos >= 16 || s_room - pos >= 16);
            if constexpr (SL)
                v[u] = whole ? lds_ld16a((const lds_u8*)(s + pos)) : u32x4{0, 0, 0, 0};
            else
                v[u] = whole ? ld16(s + pos) : u32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int64_t pos = base + 16 * kWave * u + 16 * (int64_t)lane;
            if (pos < len) {
                if (len - pos >= 16 || (d_room - pos >= 16 && s_room - pos >= 16)) {
                    st16(d + pos, v[u]);
                } else {
                    for (int64_t k = pos; k < len; ++k) d[k] = s[k];
                }
            }
        }
    }
}

}  // namespace lz4m

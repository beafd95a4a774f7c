// lz4m_sizes.hip -- batched decoded-size pass for MI355X (gfx950).
//
// size[i] = what LZ4_decompress_safe(src_i, dst, src_len[i], cap) returns once
// cap is large enough not to matter (any cap >= 255 * src_len + 64), or what
// LZ4_decompress_safe_usingDict returns with dict_len[i] bytes of dictionary:
// the decoded size, or -(error position) - 1.  The token stream alone fixes
// it, so the pass reads the compressed bytes once and writes 4 bytes a block.
//
// With the capacity out of the way the reference's state machine (lz4.c:1996-
// 2329, restated by decode_step in lz4m_decompress.hip) loses its state: the
// fast loop and the safe loop then take the same decisions for every
// sequence, so one step function of (ip, op) is exact (size_step below):
//   - a literal length below 15 with the token at ip <= iend - 18 is skipped
//     without an end test (the fast loop, lz4.c:2034, and the safe loop's
//     shortcut, lz4.c:2128, agree);
//   - any other literal ends the block when it runs past iend - 8: exactly to
//     iend is the block's end, anything else the error (lz4.c:2172-2229);
//   - the match length is read with read_variable_length(iend - 4), then the
//     window test offset > op + dictionary (dictionaries below 64 KiB only);
//     offset 0 is not an error, as in the decoders.
// A size above INT32_MAX reports LZ4M_SIZE_OVERFLOW: the output position is
// kept in 64 bits (it cannot overflow them: 255 per input byte), so the test
// is made once, when the block ends or fails.
//
// Two walks:
//   lane -- one lane per block (large batches).  The stream bytes are staged
//           in a 128-byte LDS ring per lane, refilled in aligned 64-byte
//           pieces; the common sequence (literal <= 12 bytes, at most one
//           match-length byte below 255, 20 bytes before the input's end) is
//           taken straight from the ring, anything else by size_step on the
//           same lane.
//   wave -- one wavefront per block (few large blocks).  The wave stages the
//           input in a 2 KiB LDS ring, 1 KiB per refill, requested one refill
//           ahead.  Every lane parses the sequence that would start at its
//           byte of the next 64; the chain of real starts is followed by
//           readlane, a prefix sum of lit + ml along it gives each
//           sequence's output position for the window test, and the first
//           sequence that is not common (here: a length byte of 255, or the
//           input's last 16 bytes) goes to size_step, run by the wave with
//           uniform operands.  A length run that fills 16 bytes is read
//           by the whole wave, 1 KiB per round trip.  Literals are skipped,
//           so the ring restarts wherever the stream goes on.
// Neither takes scratch: blocks are assigned statically by a grid-stride loop.
#include "lz4m_common.h"
#include "../../include/lz4m.h"

namespace lz4m {
namespace {

constexpr int64_t kSizeMax = 0x7FFFFFFF;
// AUTO: the lane walk from here.  Measured with 64 KiB blocks (tools/bench_sizes.py, profiles/sizes_bench.json):
// the wave walk is the faster one up to 16 384 blocks (2.94 against 3.99 ms), the lane walk from 24 576 (4.06
// against 4.11 ms), and the lane walk's time hardly grows from there (4.29 ms at 131 072 blocks).
constexpr int kLaneMinBlocks = 24576;

typedef __attribute__((address_space(3))) uint32_t lds_u32;

__device__ __forceinline__ int32_t final_status(bool failed, int64_t ip, int64_t op) {
    if (op > kSizeMax) return LZ4M_SIZE_OVERFLOW;
    return failed ? (int32_t)(-ip - 1) : (int32_t)op;
}

// One sequence of the block at (ip, op), exact.  in16(p): the 16 stream bytes
// at p, zero at and beyond iend; run: read_variable_length (len_run's
// contract).  Returns true when the block is over: `failed` tells how, and ip
// is then the reference's error position.
template <typename In16, typename Run>
__device__ __forceinline__ bool size_step(In16&& in16, Run&& run, int64_t iend, int64_t dlen, int64_t& ip,
                                          int64_t& op, bool& failed) {
    const u32x4 w = in16(ip);
    const uint32_t tok = w.x & 0xFFu;
    int64_t p = ip + 1, lit = tok >> 4, ml = tok & 15u, add = 0;
    uint32_t off;
    failed = false;
    if (lit < 15 && p <= iend - 17) {   // lz4.c:2034 / :2128: no end test
        off = lit <= 13 ? (window_dword(w, (uint32_t)(1 + lit)) & 0xFFFFu) : (in16(p + lit).x & 0xFFFFu);
        p += lit;
    } else {
        if (lit == 15) {
            if (!run(p, iend - 15, true, add)) goto fail;
            lit += add;
        }
        if (p + lit > iend - 8) {   // lz4.c:2172-2229
            if (p + lit != iend) goto fail;
            op += lit;
            ip = iend;
            return true;
        }
        p += lit;
        off = in16(p).x & 0xFFFFu;
    }
    op += lit;
    p += 2;
    if (ml == 15) {
        if (!run(p, iend - 4, false, add)) goto fail;
        ml += add;
    }
    ml += 4;
    if (dlen < 65536 && (int64_t)off > op + dlen) goto fail;   // lz4.c:2071 / :2248
    op += ml;
    ip = p;
    return false;
fail:
    failed = true;
    ip = p;
    return true;
}

// ------------------------------------------------------------- lane walk
constexpr int kLW = 128;       // ring bytes per lane
constexpr int kLStride = 33;   // ring stride in dwords: lanes at the same ring offset hit different banks
constexpr int kLSteps = 4;     // common sequences per look at the ring's fill

__device__ __forceinline__ void lane_ring_put(lds_u32* W, int32_t h, const uint8_t* s, int64_t x, int64_t iend) {
    u32x4 v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int64_t y = x + 16 * c;
        v[c] = y + 16 <= iend ? ld16(s + y) : ld16_guarded(s + y, iend - y);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {   // dword stores: the ring is 4-byte aligned only
        W[16 * h + 4 * c + 0] = v[c].x;
        W[16 * h + 4 * c + 1] = v[c].y;
        W[16 * h + 4 * c + 2] = v[c].z;
        W[16 * h + 4 * c + 3] = v[c].w;
    }
}

__global__ __launch_bounds__(64) void sizes_lane_kernel(const uint8_t* __restrict__ src,
                                                        const int64_t* __restrict__ src_off,
                                                        const int32_t* __restrict__ src_len,
                                                        const int32_t* __restrict__ dict_len,
                                                        int32_t* __restrict__ size, int64_t n) {
    __shared__ uint32_t rings[64 * kLStride];
    lds_u32* W = (lds_u32*)(rings + threadIdx.x * kLStride);
    const lds_u8* Wb = (const lds_u8*)W;
    for (int64_t base = (int64_t)blockIdx.x * 64; base < n; base += (int64_t)gridDim.x * 64) {
        const int64_t i = base + threadIdx.x;
        const uint8_t* s = nullptr;
        int64_t iend = 0, ip = 0, op = 0, dlen = 0, wb = 0;
        int32_t sh = 0;
        bool live = false;
        if (i < n) {
            const int64_t so = src_off[i];
            const int32_t il = src_len[i];
            if (il <= 0) {
                size[i] = -1;   // lz4.c:1983
            } else {
                // positions are kept shifted by sh = the block's offset in its
                // 64-byte line, so that every ring refill is one aligned 64-byte
                // piece; the bytes before the block are read, never parsed, and
                // only where they lie inside the caller's buffer
                sh = (int32_t)((uintptr_t)(src + so) & 63u);
                if (so < sh) sh = 0;
                s = src + so - sh;
                iend = (int64_t)il + sh;
                ip = sh;
                dlen = dict_len ? dict_len[i] : 0;
                if (dlen < 0) dlen = 0;
                wb = -4 * kLW;
                live = true;
            }
        }
        const bool check = dlen < 65536;
        while (__any(live)) {
            if (live) {
                if (ip + 32 > wb + kLW && wb + kLW < iend) {   // the ring ends within 32 bytes: refill
                    const int64_t nb = ip & ~(int64_t)63;
                    if (nb == wb + 64) {
                        lane_ring_put(W, (int32_t)(wb >> 6) & 1, s, wb + kLW, iend);
                        wb += 64;
                    } else {
                        lane_ring_put(W, (int32_t)(nb >> 6) & 1, s, nb, iend);
                        lane_ring_put(W, (int32_t)((nb >> 6) + 1) & 1, s, nb + 64, iend);
                        wb = nb;
                    }
                }
                // the common sequence from the ring: the token byte, then the
                // aligned dword pair holding the offset and the match-length byte.
                // ip <= iend - 20 with at most 16 bytes a sequence covers every
                // end test of size_step's first branch and both length reads.
                const int64_t lim = min(wb + kLW - 16, iend - 20);
                bool go = ip >= wb, any = false;
    #pragma unroll
                for (int u = 0; u < kLSteps; ++u) {
                    const uint32_t x = (uint32_t)ip;
                    const uint32_t tok = Wb[x & (kLW - 1)];
                    const uint32_t lit = tok >> 4, mlc = tok & 15u;
                    const uint32_t ob = x + 1 + lit;
                    const uint32_t lo = W[(ob & (kLW - 4)) >> 2], hi = W[((ob + 4) & (kLW - 4)) >> 2];
                    const uint32_t dw = __builtin_amdgcn_alignbyte(hi, lo, ob);
                    const bool mlx = mlc == 15u;
                    const uint32_t e = (dw >> 16) & 0xFFu;
                    const int64_t off = dw & 0xFFFFu;
                    const int64_t ol = op + lit;
                    const bool take = go & (ip <= lim) & (lit <= 12u) & !(mlx & (e == 255u)) & (!check | (off <= ol + dlen));
                    ip += take ? (int64_t)(3u + lit + (mlx ? 1u : 0u)) : 0;
                    op = take ? ol + mlc + 4 + (mlx ? e : 0u) : op;
                    any |= take;
                    go = take;
                }
                if (!any) {
                    bool failed = false;
                    auto in16 = [&](int64_t p) { return ld16_guarded(s + p, iend - p); };
                    auto run = [&](int64_t& p, int64_t lim2, bool init, int64_t& add) {
                        return len_run(in16, p, lim2, init, add);
                    };
                    if (size_step(in16, run, iend, dlen, ip, op, failed)) {
                        size[i] = final_status(failed, ip - sh, op);
                        live = false;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------- wave walk
constexpr int kWH = 1024;          // ring half: one refill, 16 bytes a lane
constexpr int kWR = 2 * kWH;       // ring bytes
constexpr int kWPad = 32;          // the ring's first bytes again after its end: 16-byte reads across the wrap
constexpr int kWSpan = 64 + 2 + 269 + 8;   // bytes a round may read from ip on: a start byte, its literal, a dword pair

__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ u32x4 wave_load_half(const uint8_t* s, int64_t x, int64_t iend, uint32_t lane) {
    const int64_t y = x + 16 * (int64_t)lane;
    return y + 16 <= iend ? ld16(s + y) : ld16_guarded(s + y, iend - y);
}
__device__ __forceinline__ void wave_put_half(lds_u8* R, int32_t h, u32x4 v, uint32_t lane) {
    lds_st16(R + kWH * h + 16 * lane, v);
    if (h == 0 && lane < kWPad / 16) lds_st16(R + kWR + 16 * lane, v);
}

// The 4 ring bytes of stream position x (any alignment), from the aligned dword pair holding them.
__device__ __forceinline__ uint32_t ring_dword(const lds_u8* R, uint32_t x) {
    const lds_cu32a* q = (const lds_cu32a*)(R + (x & (kWR - 4)));
    return __builtin_amdgcn_alignbyte(q[1], q[0], x);
}

// read_variable_length by the whole wave (uniform arguments), 1 KiB per round
// trip: len_run's outcome (its 16 bytes a step are this one's 1024).
__device__ __forceinline__ bool wave_len_run(const uint8_t* s, int64_t iend, int64_t& ip, int64_t ilimit,
                                             bool initial_check, int64_t& out, uint32_t lane) {
    if (initial_check && ip >= ilimit) return false;
    if (ip >= ilimit) {
        ++ip;
        return false;
    }
    int64_t len = 0;
    for (;;) {
        const u32x4 v = wave_load_half(s, ip, iend, lane);
        const uint32_t n0 = ~v.x, n1 = ~v.y, n2 = ~v.z, n3 = ~v.w;
        const uint32_t q = n0 ? 0u : n1 ? 1u : n2 ? 2u : n3 ? 3u : 4u;
        const uint32_t nw = q == 0 ? n0 : q == 1 ? n1 : q == 2 ? n2 : n3;
        const uint32_t bi = q < 4 ? (uint32_t)__builtin_ctz(nw) >> 3 : 0u;
        const uint64_t hit = __ballot(q < 4);
        if (hit != 0) {
            const int fl = __builtin_ctzll(hit);
            const int64_t j = 16 * fl + rdl((int32_t)(4 * q + bi), fl);   // first byte != 255
            if (ip + j >= ilimit) {
                ip = ilimit + 1;
                return false;
            }
            len += 255 * j + rdl((int32_t)((~nw >> (8 * bi)) & 0xFFu), fl);
            ip += j + 1;
            out = len;
            return true;
        }
        if (ip + 16 * kWave > ilimit) {   // the run reaches ilimit
            ip = ilimit + 1;
            return false;
        }
        len += 255 * 16 * kWave;
        ip += 16 * kWave;
    }
}

__global__ __launch_bounds__(256) void sizes_wave_kernel(const uint8_t* __restrict__ src,
                                                         const int64_t* __restrict__ src_off,
                                                         const int32_t* __restrict__ src_len,
                                                         const int32_t* __restrict__ dict_len,
                                                         int32_t* __restrict__ size, int64_t n) {
    __shared__ __attribute__((aligned(16))) uint8_t rings[4][kWR + kWPad];
    const uint32_t lane = lane_id();
    const uint32_t wave = uni(threadIdx.x >> 6);
    lds_u8* R = (lds_u8*)rings[wave];
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < n; b += (int64_t)gridDim.x * 4) {
        const int64_t iend = src_len[b];
        if (iend <= 0) {
            if (lane == 0) size[b] = -1;   // lz4.c:1983
            continue;
        }
        const uint8_t* s = src + src_off[b];
        int64_t dlen = dict_len ? dict_len[b] : 0;
        if (dlen < 0) dlen = 0;
        const bool check = dlen < 65536;
        int64_t ip = 0, op = 0, wb = -4 * kWR;
        u32x4 pf = u32x4{0, 0, 0, 0};   // stream bytes [wb + kWR, wb + kWR + kWH), requested ahead
        bool failed = false;
        for (;;) {
            if (ip + kWSpan > wb + kWR) {   // the ring ends inside this round's reads
                const int64_t nb = ip & ~(int64_t)(kWH - 1);
                if (nb == wb + kWH) {
                    wave_put_half(R, (int32_t)(wb >> 10) & 1, pf, lane);
                } else {
                    const u32x4 a = wave_load_half(s, nb, iend, lane), c = wave_load_half(s, nb + kWH, iend, lane);
                    wave_put_half(R, (int32_t)(nb >> 10) & 1, a, lane);
                    wave_put_half(R, (int32_t)((nb >> 10) + 1) & 1, c, lane);
                }
                wb = nb;
                pf = wave_load_half(s, wb + kWR, iend, lane);
                lds_wait();
            }
            // every lane: the sequence that would start at byte ip + lane.  The token and the first
            // literal-length byte from the aligned dword pair at that byte, the offset and the first
            // match-length byte from the pair after the literal (at most 269 bytes on: inside the ring).
            // ip + adv <= iend - 16 covers every end test size_step makes for such a sequence.
            const int64_t ipl = ip + lane;
            const uint32_t x0 = ring_dword(R, (uint32_t)ipl);
            const uint32_t tok = x0 & 0xFFu, mlc = tok & 15u, b = (x0 >> 8) & 0xFFu;
            const bool litx = (tok >> 4) == 15u, mlx = mlc == 15u;
            const uint32_t lit = (tok >> 4) + (litx ? b : 0u), hdr = litx ? 2u : 1u;
            const uint32_t dw = ring_dword(R, (uint32_t)ipl + hdr + lit);
            const int64_t off = dw & 0xFFFFu;
            const uint32_t e = (dw >> 16) & 0xFFu;
            const int32_t len = (int32_t)(hdr + lit + 2u + (mlx ? 1u : 0u));
            const bool common = !(litx & (b == 255u)) & !(mlx & (e == 255u)) & (ipl + len <= iend - 16);
            const int32_t adv = common ? len : 0;
            const int32_t outb = (int32_t)(lit + mlc + 4u + (mlx ? e : 0u));
            // the chain of real starts from lane 0, up to the first start that is not common
            uint64_t chain = 0;
            int32_t cur = 0;
            while (cur < kWave) {
                const int32_t a = rdl(adv, cur);
                if (a == 0) break;
                chain |= 1ull << cur;
                cur += a;
            }
            const bool on = (chain >> lane) & 1ull;
            const int32_t v = on ? outb : 0;
            const int32_t incl = wave_incl_sum(v);
            const int64_t opl = op + (incl - v);   // the output position before this lane's sequence
            const uint64_t bad = __ballot(on & check & (off > opl + lit + dlen));
            bool exact = cur < kWave;
            if (bad != 0) {   // the first sequence that fails the window test: size_step reports it
                const int f = __builtin_ctzll(bad);
                ip += f;
                op += rdl(incl - v, f);
                exact = true;
            } else {
                ip += cur;
                op += rdl(incl, kWave - 1);
            }
            if (!exact) continue;
            auto in16 = [&](int64_t p) {
                if (p >= wb && p + 16 <= wb + kWR) return lds_ld16a(R + ((uint32_t)p & (kWR - 1)));
                return ld16_guarded(s + p, iend - p);
            };
            auto run = [&](int64_t& p, int64_t lim, bool init, int64_t& add) {
                const u32x4 h = in16(p);
                if ((h.x & h.y & h.z & h.w) != 0xFFFFFFFFu) return len_run(in16, p, lim, init, add);
                return wave_len_run(s, iend, p, lim, init, add, lane);
            };
            const bool over = size_step(in16, run, iend, dlen, ip, op, failed);
            ip = readlane64(ip, 0);
            op = readlane64(op, 0);
            if (over) break;
        }
        if (lane == 0) size[b] = final_status(failed, ip, op);
    }
}

}  // namespace
}  // namespace lz4m

extern "C" int lz4m_decompressed_size_batch(const uint8_t* d_src, const int64_t* d_src_off, const int32_t* d_src_len,
                                            const int32_t* d_dict_len, int32_t* d_size, int64_t n, int walk,
                                            lz4m_stream_t stream) {
    using namespace lz4m;
    if (n < 0 || !(walk == LZ4M_WALK_AUTO || walk == LZ4M_WALK_LANE || walk == LZ4M_WALK_WAVE)) return LZ4M_EINVAL;
    if (n == 0) return 0;
    if (walk == LZ4M_WALK_AUTO) walk = n >= kLaneMinBlocks ? LZ4M_WALK_LANE : LZ4M_WALK_WAVE;
    hipStream_t st = (hipStream_t)stream;
    if (walk == LZ4M_WALK_LANE) {
        const int64_t grid = (n + 63) / 64;
        hipLaunchKernelGGL(sizes_lane_kernel, dim3((uint32_t)(grid < (1 << 20) ? grid : (1 << 20))), dim3(64), 0, st,
                           d_src, d_src_off, d_src_len, d_dict_len, d_size, n);
    } else {
        const int64_t grid = (n + 3) / 4;
        hipLaunchKernelGGL(sizes_wave_kernel, dim3((uint32_t)(grid < 65536 ? grid : 65536)), dim3(256), 0, st, d_src,
                           d_src_off, d_src_len, d_dict_len, d_size, n);
    }
    return (int)hipGetLastError();
}

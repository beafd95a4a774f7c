// lz4m_frames.hip -- the per-frame layer of batched LZ4 frames (gfx950).
//
// A batch is n complete frames in one device buffer.  Everything that is
// serial inside one frame -- parsing its header, walking its block records
// (each record's position depends on the previous one's size), writing its
// header and endmark -- runs on one lane per frame, the frames side by side;
// everything per block (compression, decoding, record emission, checksums)
// runs in the block-batched launchers over the blocks of all frames at once.
//   one frame: frame_scan (lz4.frame.decompress_device), the same walk
//   decode:   frames_scan (count the records) -> exclusive scan of the counts
//             -> frames_records (fill the global per-block arrays)
//   compress: frames_plan (block-size id, block count, linked) -> scan ->
//             frames_plan_blocks (one lane per block) -> compress, record
//             sizes, scan -> frames_sizes -> scan -> frames_emit
// The linked chains themselves decode in lz4m_decompress.hip
// (lz4m_decompress_chains), next to the single-chain body they share.
#include "lz4m_common.h"
#include "../../include/lz4m.h"
#include "lz4m_xxh32_dev.h"

namespace lz4m {

constexpr uint32_t kFrameMagic = 0x184D2204u, kSkipMagic = 0x184D2A50u;

__device__ __forceinline__ int64_t bsid_bytes(int bsid) { return (int64_t)1 << (8 + 2 * bsid); }   // 4 -> 64 KiB

// the header checksum byte (lz4frame.c:341-345): the descriptor is 2..14
// bytes, below one XXH32 stripe, so the hash is the short-input path
// (xxhash.c:381-389) with seed 0
__device__ __forceinline__ uint8_t header_checksum(const uint8_t* desc, int len) {
    return (uint8_t)(xfinish(kP5 + (uint32_t)len, desc, len) >> 8);
}

struct FrameHead {
    int32_t status, hsize, bsid, flags;
    int64_t content_size, end;
};

// LZ4F_headerSize + LZ4F_decodeHeader (lz4frame.c:1291-1380, 1387-1463), in
// the order lz4.frame's _parse_header checks them
__device__ FrameHead parse_head(const uint8_t* p, int64_t n) {
    FrameHead h{LZ4M_FRAME_OK, 0, 0, 0, 0, 0};
    if (n < 5) {
        h.status = LZ4M_FRAME_HEADER_INCOMPLETE;
        return h;
    }
    const uint32_t magic = ld32(p);
    if ((magic & 0xFFFFFFF0u) == kSkipMagic) {   // lz4frame.c:1303-1311
        if (n < 8) {
            h.status = LZ4M_FRAME_HEADER_INCOMPLETE;
            return h;
        }
        h.hsize = 8;
        const int64_t end = 8 + (int64_t)ld32(p + 4);
        h.status = n < end ? LZ4M_FRAME_TRUNCATED : LZ4M_FRAME_SKIPPABLE;
        h.end = n < end ? n : end;
        return h;
    }
    if (magic != kFrameMagic) {
        h.status = LZ4M_FRAME_MAGIC_UNKNOWN;
        return h;
    }
    const uint32_t flg = p[4];
    h.hsize = 7 + ((flg & 0x08u) ? 8 : 0) + ((flg & 0x01u) ? 4 : 0);
    if (n < h.hsize) {
        h.status = LZ4M_FRAME_HEADER_INCOMPLETE;
        return h;
    }
    if ((flg >> 1) & 1u) {
        h.status = LZ4M_FRAME_RESERVED_FLAG;
        return h;
    }
    if (((flg >> 6) & 3u) != 1u) {
        h.status = LZ4M_FRAME_VERSION_WRONG;
        return h;
    }
    const uint32_t bd = p[5];
    h.bsid = (int32_t)((bd >> 4) & 7u);
    if ((bd >> 7) & 1u) {
        h.status = LZ4M_FRAME_RESERVED_FLAG;
        return h;
    }
    if (h.bsid < 4) {
        h.status = LZ4M_FRAME_BLOCK_SIZE_ID;
        return h;
    }
    if (bd & 0x0Fu) {
        h.status = LZ4M_FRAME_RESERVED_FLAG;
        return h;
    }
    if (header_checksum(p + 4, h.hsize - 5) != p[h.hsize - 1]) {
        h.status = LZ4M_FRAME_HEADER_CHECKSUM;
        return h;
    }
    h.flags = (((flg >> 5) & 1u) ? 0 : LZ4M_FRAME_LINKED) | (((flg >> 4) & 1u) ? LZ4M_FRAME_BLOCK_CHECKSUM : 0) |
              (((flg >> 2) & 1u) ? LZ4M_FRAME_CONTENT_CHECKSUM : 0) | ((flg & 0x08u) ? LZ4M_FRAME_CONTENT_SIZE : 0) |
              ((flg & 0x01u) ? LZ4M_FRAME_DICT_ID : 0);
    if (flg & 0x08u) h.content_size = (int64_t)ld64(p + 6);
    return h;
}

// not a frame status: walk_records<true> stopped at `limit` records, before an endmark
constexpr int32_t kWalkAtLimit = -1;

// LZ4F_decompress's walk over the block records (lz4frame.c:1643-1701 block
// headers, 1926-1965 endmark and content checksum) from `pos` of a frame of n
// bytes at p: the one walk of the tree, for one frame (frame_scan_kernel) and
// for a batch (frames_scan_kernel counts, frames_records_kernel stores).
// Serial by construction -- each record's position depends on the previous
// one's size -- so one lane walks a frame: one dependent HBM read per record
// (measured 0.25 us per record, stores included: 4 ms for the 16 384 records
// of a 1 GiB frame of 64 KiB blocks, profiles/frame_refactor.json).
// EMIT: store record k's fields at base + k (rec_crc too if CRC), at most
// `limit` records.
template <bool EMIT, bool CRC = EMIT>
__device__ __forceinline__ int32_t walk_records(const uint8_t* p, int64_t n, int64_t pos, int crc,
                                                int content_checksum, int64_t max_block, int32_t& status,
                                                int64_t& end, int64_t& cpos, int64_t abs, int64_t base,
                                                int64_t* rec_pos, int32_t* rec_len, uint8_t* rec_raw,
                                                int64_t* rec_crc, int64_t limit) {
    int64_t k = 0;
    status = LZ4M_FRAME_OK;
    end = 0;
    cpos = -1;
    while (true) {
        if (n - pos < 4) {
            status = LZ4M_FRAME_TRUNCATED;
            break;
        }
        const uint32_t hdr = ld32(p + pos);
        pos += 4;
        if (hdr == 0) {   // endmark
            if (content_checksum) {
                if (n - pos < 4) {
                    status = LZ4M_FRAME_CONTENT_CHECKSUM_MISSING;
                    break;
                }
                cpos = pos;
                end = pos + 4;
            } else {
                end = pos;
            }
            break;
        }
        const int64_t size = hdr & 0x7FFFFFFFu;
        if (size > max_block) {
            status = LZ4M_FRAME_BLOCK_TOO_LARGE;
            break;
        }
        if (n - pos < size + crc || k == 0x7FFFFFFF) {
            status = LZ4M_FRAME_TRUNCATED;
            break;
        }
        if (EMIT) {
            if (k == limit) {   // never past the caller's arrays (the count the first pass took)
                status = kWalkAtLimit;
                break;
            }
            rec_pos[base + k] = abs + pos;
            rec_len[base + k] = (int32_t)size;
            rec_raw[base + k] = (uint8_t)(hdr >> 31);
            if (CRC) rec_crc[base + k] = crc ? abs + pos + size : -1;
        }
        ++k;
        pos += size + crc;
    }
    return (int32_t)k;
}

// lz4m_frame_scan: one frame, one lane.  result = {records, state, end,
// content-checksum position}, the state as include/lz4m.h documents it.
// The records' checksum positions (rec_crc, may be null) follow from their
// positions and sizes and are filled by the whole workgroup after the walk: the
// walk waits for its stores with each dependent read, and a fourth store in its
// loop measured +28 ns on 245 ns per record.
__global__ __launch_bounds__(256) void frame_scan_kernel(const uint8_t* __restrict__ frame, int64_t n, int64_t pos,
                                                         int crc, int content_checksum, int32_t max_block,
                                                         int64_t max_rec, int64_t* __restrict__ rec_pos,
                                                         int32_t* __restrict__ rec_len, uint8_t* __restrict__ rec_raw,
                                                         int64_t* __restrict__ rec_crc,
                                                         int64_t* __restrict__ result) {
    __shared__ int32_t records;
    if (threadIdx.x == 0) {
        int32_t st;
        int64_t end, cpos;
        records = walk_records<true, false>(frame, n, pos, crc, content_checksum, max_block, st, end, cpos, 0, 0,
                                            rec_pos, rec_len, rec_raw, nullptr, max_rec);
        result[0] = records;
        result[1] = st == LZ4M_FRAME_OK ? 0 : st == LZ4M_FRAME_TRUNCATED ? 1 : st == LZ4M_FRAME_BLOCK_TOO_LARGE ? 2
                  : st == LZ4M_FRAME_CONTENT_CHECKSUM_MISSING ? 3 : 4;   // 4: kWalkAtLimit, more than max_rec records
        result[2] = end;
        result[3] = cpos;
    }
    if (rec_crc == nullptr) return;
    __syncthreads();   // (orders lane 0's stores before the workgroup's reads of them)
    for (int32_t k = threadIdx.x; k < records; k += blockDim.x) rec_crc[k] = crc ? rec_pos[k] + rec_len[k] : -1;
}

__global__ __launch_bounds__(64) void frames_scan_kernel(const uint8_t* __restrict__ buf,
                                                         const int64_t* __restrict__ frame_off,
                                                         const int64_t* __restrict__ frame_len, int64_t n,
                                                         int32_t* __restrict__ status, int32_t* __restrict__ nblocks,
                                                         int32_t* __restrict__ hsize, int64_t* __restrict__ end,
                                                         int64_t* __restrict__ cpos, int32_t* __restrict__ bsid,
                                                         int32_t* __restrict__ flags,
                                                         int64_t* __restrict__ content_size) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = buf + frame_off[i];
    const int64_t len = frame_len[i] < 0 ? 0 : frame_len[i];
    FrameHead h = parse_head(p, len);
    int32_t k = 0;
    int64_t cp = -1;
    if (h.status == LZ4M_FRAME_OK) {
        int32_t st;
        k = walk_records<false>(p, len, h.hsize, (h.flags & LZ4M_FRAME_BLOCK_CHECKSUM) ? 4 : 0,
                                h.flags & LZ4M_FRAME_CONTENT_CHECKSUM, bsid_bytes(h.bsid), st, h.end, cp, 0, 0,
                                nullptr, nullptr, nullptr, nullptr, 0);
        h.status = st;
        if (st != LZ4M_FRAME_OK) k = 0;   // a malformed frame decodes nothing
    }
    status[i] = h.status;
    nblocks[i] = k;
    hsize[i] = h.hsize;
    end[i] = h.end;
    cpos[i] = cp < 0 ? -1 : frame_off[i] + cp;
    bsid[i] = h.bsid;
    flags[i] = h.flags;
    content_size[i] = h.content_size;
}

__global__ __launch_bounds__(64) void frames_records_kernel(
    const uint8_t* __restrict__ buf, const int64_t* __restrict__ frame_off, const int64_t* __restrict__ frame_len,
    const int32_t* __restrict__ nblocks, const int32_t* __restrict__ hsize, const int32_t* __restrict__ bsid,
    const int32_t* __restrict__ flags, const int64_t* __restrict__ block_base, const int64_t* __restrict__ slot_base,
    int64_t n, int64_t* __restrict__ rec_pos, int32_t* __restrict__ rec_len, uint8_t* __restrict__ rec_raw,
    int64_t* __restrict__ rec_crc, int64_t* __restrict__ rec_frame, int64_t* __restrict__ slot_off,
    int32_t* __restrict__ slot_cap) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t nb = nblocks[i];
    if (nb <= 0) return;
    const int64_t base = block_base[i];
    const int64_t maxb = bsid_bytes(bsid[i]);
    int32_t st;
    int64_t e, c;
    walk_records<true>(buf + frame_off[i], frame_len[i], hsize[i], (flags[i] & LZ4M_FRAME_BLOCK_CHECKSUM) ? 4 : 0,
                       flags[i] & LZ4M_FRAME_CONTENT_CHECKSUM, maxb, st, e, c, frame_off[i], base, rec_pos, rec_len,
                       rec_raw, rec_crc, nb);
    for (int64_t k = 0; k < nb; ++k) {
        rec_frame[base + k] = i;
        slot_off[base + k] = slot_base[i] + k * maxb;
        slot_cap[base + k] = (int32_t)maxb;
    }
}

// ---------------------------------------------------------------- compress
// LZ4F_optimalBSID (lz4frame.c:351-363), then the default id and the linked
// rule of LZ4F_compressFrame (lz4frame.c:436-442).  bsid -1: not a block size.
__global__ __launch_bounds__(64) void frames_plan_kernel(const int64_t* __restrict__ src_len, int64_t n,
                                                         int32_t requested, int32_t linked_req,
                                                         int32_t* __restrict__ bsid, int32_t* __restrict__ nblocks,
                                                         int32_t* __restrict__ linked) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t len = src_len[i];
    int32_t id = requested, proposed = 4;
    int64_t max_size = 64 << 10;
    while (requested > proposed && proposed <= 7) {   // past 7 the result is no block size either way
        if (len <= max_size) {
            id = proposed;
            break;
        }
        ++proposed;
        max_size <<= 2;
    }
    if (id == 0) id = 4;   // LZ4F_BLOCKSIZEID_DEFAULT
    if (id < 4 || id > 7 || len < 0) {
        bsid[i] = -1;
        nblocks[i] = 0;
        linked[i] = 0;
        return;
    }
    const int64_t bs = bsid_bytes(id);
    const int64_t nb = (len + bs - 1) / bs;
    bsid[i] = nb > 0x7FFFFFFF ? -1 : id;
    nblocks[i] = nb > 0x7FFFFFFF ? 0 : (int32_t)nb;
    linked[i] = linked_req && len > bs;   // lz4frame.c:441-442
}

// one lane per block; its frame is found by bisection of block_base (n + 1
// ascending entries, empty frames repeat an entry)
__global__ __launch_bounds__(256) void frames_plan_blocks_kernel(
    const int64_t* __restrict__ src_off, const int64_t* __restrict__ src_len, const int32_t* __restrict__ bsid,
    const int32_t* __restrict__ linked, const int64_t* __restrict__ block_base, int64_t n, int64_t total,
    int64_t* __restrict__ raw_off, int32_t* __restrict__ raw_len, int32_t* __restrict__ cap,
    int32_t* __restrict__ link, int32_t* __restrict__ hist, int64_t* __restrict__ owner,
    int32_t* __restrict__ slot_len) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= total) return;
    int64_t lo = 0, hi = n;   // the last frame with block_base <= b
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (block_base[mid] <= b) lo = mid;
        else hi = mid;
    }
    const int64_t f = lo, k = b - block_base[f];
    const int64_t bs = bsid_bytes(bsid[f]);
    const int64_t at = k * bs, left = src_len[f] - at;
    const int32_t len = (int32_t)(left < bs ? left : bs);
    raw_off[b] = src_off[f] + at;
    raw_len[b] = len;
    cap[b] = len - 1;   // lz4frame.c:835
    link[b] = linked[f] && k > 0;
    hist[b] = linked[f] ? (int32_t)(at < 65536 ? at : 65536) : 0;
    owner[b] = f;
    slot_len[b] = len + len / 255 + 16;   // LZ4_compressBound
}

__global__ __launch_bounds__(64) void frames_sizes_kernel(const int64_t* __restrict__ rec_off,
                                                          const int64_t* __restrict__ block_base,
                                                          const int64_t* __restrict__ src_len, int store_size,
                                                          int content_checksum, int64_t n,
                                                          int32_t* __restrict__ hsize,
                                                          int64_t* __restrict__ frame_size) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t h = 7 + (store_size && src_len[i] > 0 ? 8 : 0);
    hsize[i] = h;
    frame_size[i] = h + (rec_off[block_base[i + 1]] - rec_off[block_base[i]]) + 4 + (content_checksum ? 4 : 0);
}

__device__ __forceinline__ void put32(uint8_t* d, uint32_t v) {
    d[0] = (uint8_t)v;
    d[1] = (uint8_t)(v >> 8);
    d[2] = (uint8_t)(v >> 16);
    d[3] = (uint8_t)(v >> 24);
}

// LZ4F_compressBegin_usingCDict's header (lz4frame.c:752-780), the endmark
// (lz4frame.c:1167) and the content checksum (lz4frame.c:1170-1176)
__global__ __launch_bounds__(64) void frames_emit_kernel(uint8_t* __restrict__ frames,
                                                         const int64_t* __restrict__ frame_off,
                                                         const int64_t* __restrict__ frame_size,
                                                         const int32_t* __restrict__ bsid,
                                                         const int32_t* __restrict__ linked,
                                                         const int64_t* __restrict__ src_len, int store_size,
                                                         int block_checksum, int content_checksum,
                                                         const uint32_t* __restrict__ content_hash, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t* d = frames + frame_off[i];
    const bool sized = store_size && src_len[i] > 0;
    put32(d, kFrameMagic);
    d[4] = (uint8_t)((1u << 6) | ((linked[i] ? 0u : 1u) << 5) | ((block_checksum ? 1u : 0u) << 4) |
                     ((sized ? 1u : 0u) << 3) | ((content_checksum ? 1u : 0u) << 2));
    d[5] = (uint8_t)((bsid[i] & 7) << 4);
    int h = 6;
    if (sized) {
        const uint64_t v = (uint64_t)src_len[i];
        put32(d + 6, (uint32_t)v);
        put32(d + 10, (uint32_t)(v >> 32));
        h = 14;
    }
    d[h] = header_checksum(d + 4, h - 4);   // over the bytes this lane just wrote
    uint8_t* t = d + frame_size[i] - 4 - (content_checksum ? 4 : 0);
    put32(t, 0u);
    if (content_checksum) put32(t + 4, content_hash[i]);
}

}  // namespace lz4m

using namespace lz4m;

namespace {
inline dim3 lanes(int64_t n, int per) { return dim3((uint32_t)((n + per - 1) / per)); }
}

extern "C" int lz4m_frame_scan(const uint8_t* d_frame, int64_t frame_len, int64_t pos, int block_checksum,
                               int content_checksum, int32_t max_block, int64_t max_rec, int64_t* d_rec_pos,
                               int32_t* d_rec_len, uint8_t* d_rec_raw, int64_t* d_rec_crc, int64_t* d_result,
                               lz4m_stream_t stream) {
    if (frame_len < 0 || pos < 0 || max_block < 0 || max_rec < 0 || !d_result) return LZ4M_EINVAL;
    hipLaunchKernelGGL(frame_scan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d_frame, frame_len, pos,
                       block_checksum ? 4 : 0, content_checksum, max_block, max_rec, d_rec_pos, d_rec_len, d_rec_raw,
                       d_rec_crc, d_result);
    return (int)hipGetLastError();
}

extern "C" int lz4m_frames_scan(const uint8_t* d_buf, const int64_t* d_frame_off, const int64_t* d_frame_len,
                                int64_t n, int32_t* d_status, int32_t* d_nblocks, int32_t* d_hsize, int64_t* d_end,
                                int64_t* d_cpos, int32_t* d_bsid, int32_t* d_flags, int64_t* d_content_size,
                                lz4m_stream_t stream) {
    if (n < 0 || n > 0x7FFFFFFF) return LZ4M_EINVAL;
    if (n == 0) return 0;
    if (!d_frame_off || !d_frame_len || !d_status || !d_nblocks || !d_hsize || !d_end || !d_cpos ||
        !d_bsid || !d_flags || !d_content_size)
        return LZ4M_EINVAL;
    hipLaunchKernelGGL(frames_scan_kernel, lanes(n, 64), dim3(64), 0, (hipStream_t)stream, d_buf, d_frame_off,
                       d_frame_len, n, d_status, d_nblocks, d_hsize, d_end, d_cpos, d_bsid, d_flags, d_content_size);
    return (int)hipGetLastError();
}

extern "C" int lz4m_frames_records(const uint8_t* d_buf, const int64_t* d_frame_off, const int64_t* d_frame_len,
                                   const int32_t* d_nblocks, const int32_t* d_hsize, const int32_t* d_bsid,
                                   const int32_t* d_flags, const int64_t* d_block_base, const int64_t* d_slot_base,
                                   int64_t n, int64_t* d_rec_pos, int32_t* d_rec_len, uint8_t* d_rec_raw,
                                   int64_t* d_rec_crc, int64_t* d_rec_frame, int64_t* d_slot_off,
                                   int32_t* d_slot_cap, lz4m_stream_t stream) {
    if (n < 0 || n > 0x7FFFFFFF) return LZ4M_EINVAL;
    if (n == 0) return 0;
    if (!d_frame_off || !d_frame_len || !d_nblocks || !d_hsize || !d_bsid || !d_flags || !d_block_base ||
        !d_slot_base)
        return LZ4M_EINVAL;
    hipLaunchKernelGGL(frames_records_kernel, lanes(n, 64), dim3(64), 0, (hipStream_t)stream, d_buf, d_frame_off,
                       d_frame_len, d_nblocks, d_hsize, d_bsid, d_flags, d_block_base, d_slot_base, n, d_rec_pos,
                       d_rec_len, d_rec_raw, d_rec_crc, d_rec_frame, d_slot_off, d_slot_cap);
    return (int)hipGetLastError();
}

extern "C" int lz4m_frames_plan(const int64_t* d_src_len, int64_t n, int32_t block_size_id, int32_t block_linked,
                                int32_t* d_bsid, int32_t* d_nblocks, int32_t* d_linked, lz4m_stream_t stream) {
    if (n < 0 || n > 0x7FFFFFFF) return LZ4M_EINVAL;
    if (n == 0) return 0;
    if (!d_src_len || !d_bsid || !d_nblocks || !d_linked) return LZ4M_EINVAL;
    hipLaunchKernelGGL(frames_plan_kernel, lanes(n, 64), dim3(64), 0, (hipStream_t)stream, d_src_len, n,
                       block_size_id, block_linked ? 1 : 0, d_bsid, d_nblocks, d_linked);
    return (int)hipGetLastError();
}

extern "C" int lz4m_frames_plan_blocks(const int64_t* d_src_off, const int64_t* d_src_len, const int32_t* d_bsid,
                                       const int32_t* d_linked, const int64_t* d_block_base, int64_t n,
                                       int64_t n_blocks, int64_t* d_raw_off, int32_t* d_raw_len, int32_t* d_cap,
                                       int32_t* d_link, int32_t* d_hist, int64_t* d_owner, int32_t* d_slot_len,
                                       lz4m_stream_t stream) {
    if (n <= 0 || n > 0x7FFFFFFF || n_blocks < 0 || n_blocks > ((int64_t)0x7FFFFFFF << 8)) return LZ4M_EINVAL;
    if (n_blocks == 0) return 0;
    if (!d_src_off || !d_src_len || !d_bsid || !d_linked || !d_block_base || !d_raw_off || !d_raw_len || !d_cap ||
        !d_link || !d_hist || !d_owner || !d_slot_len)
        return LZ4M_EINVAL;
    hipLaunchKernelGGL(frames_plan_blocks_kernel, lanes(n_blocks, 256), dim3(256), 0, (hipStream_t)stream, d_src_off,
                       d_src_len, d_bsid, d_linked, d_block_base, n, n_blocks, d_raw_off, d_raw_len, d_cap, d_link,
                       d_hist, d_owner, d_slot_len);
    return (int)hipGetLastError();
}

extern "C" int lz4m_frames_sizes(const int64_t* d_rec_off, const int64_t* d_block_base, const int64_t* d_src_len,
                                 int store_size, int content_checksum, int64_t n, int32_t* d_hsize,
                                 int64_t* d_frame_size, lz4m_stream_t stream) {
    if (n < 0 || n > 0x7FFFFFFF) return LZ4M_EINVAL;
    if (n == 0) return 0;
    if (!d_rec_off || !d_block_base || !d_src_len || !d_hsize || !d_frame_size) return LZ4M_EINVAL;
    hipLaunchKernelGGL(frames_sizes_kernel, lanes(n, 64), dim3(64), 0, (hipStream_t)stream, d_rec_off, d_block_base,
                       d_src_len, store_size, content_checksum, n, d_hsize, d_frame_size);
    return (int)hipGetLastError();
}

extern "C" int lz4m_frames_emit(uint8_t* d_frames, const int64_t* d_frame_off, const int64_t* d_frame_size,
                                const int32_t* d_bsid, const int32_t* d_linked, const int64_t* d_src_len,
                                int store_size, int block_checksum, int content_checksum,
                                const uint32_t* d_content_hash, int64_t n, lz4m_stream_t stream) {
    if (n < 0 || n > 0x7FFFFFFF) return LZ4M_EINVAL;
    if (n == 0) return 0;
    if (!d_frames || !d_frame_off || !d_frame_size || !d_bsid || !d_linked || !d_src_len ||
        (content_checksum && !d_content_hash))
        return LZ4M_EINVAL;
    hipLaunchKernelGGL(frames_emit_kernel, lanes(n, 64), dim3(64), 0, (hipStream_t)stream, d_frames, d_frame_off,
                       d_frame_size, d_bsid, d_linked, d_src_len, store_size, block_checksum, content_checksum,
                       d_content_hash, n);
    return (int)hipGetLastError();
}

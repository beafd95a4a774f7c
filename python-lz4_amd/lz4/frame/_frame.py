"""``lz4.frame`` one-shot API on the MI355X codec.

Mirrors the reference extension ``lz4/frame/_frame.c`` (compress 112-259,
get_frame_info 640-824, __decompress 938-1193) over the frame format of
``lz4libs/lz4frame.c``.  The host walks the frame structure (header bytes,
LE32 block records); every byte-level operation runs on the GPU:

* compress: the input is cut into blocks and compressed in one batched
  launch (cap = block size - 1, raw block when it does not fit,
  lz4frame.c:834-842) -- independent blocks with the
  LZ4_compress_fast_extState_fastReset parse (lz4frame.c:853-863 ->
  lz4.c:1378-1413), linked blocks (the default) as one
  LZ4_compress_fast_continue stream (lz4frame.c:865-871), speculatively in
  parallel (lz4m_compress_linked_batch); block records are emitted by
  ``lz4m_frame_emit`` at scanned offsets.  The content checksum (XXH32 over
  all input, lz4frame.c:1042, 1171) is one serial stream: it runs on a host
  core (lz4m_xxh32_host_*) in a thread beside the device work -- on the
  caller's bytes, or on device bytes streamed back over PCIe in chunks; the
  1-byte header checksum (lz4frame.c:341-345) too.
* decompress: independent blocks decode in one batched launch into slots of
  the frame's maximum block size (the capacity LZ4F_decompress gives,
  lz4frame.c:1844-1847), raw blocks are gathered, block checksums are
  verified on the device, the content checksum on a host core.  Linked-block frames decode
  block after block on one wavefront with the previous output as prefix.

* many frames per call (compress_batch / decompress_batch on device tensors,
  compress_many / decompress_many on lists of host buffers; at the end of
  this module): the per-frame steps above run on the
  device, one lane per frame, the blocks of all frames in the same batched
  launches, linked frames one wavefront each, content checksums on the
  device.

The single-frame and the batched calls share the compression pipeline (a block
plan -- built on the host for one frame --, the block stage ``_compress_blocks``
with the parse ``resolve_parse`` made of the arguments, record sizes, a scan,
record emission: a batched frame has the single call's bytes by construction)
and the record walk (one device loop).  Separate on purpose (DESIGN.md section
10): the content hash and the decode strategy, as the two items above say.

Scope notes: every frame ``compress`` writes is byte-identical
to the reference's (``parse="parallel"`` on ``compress_device`` trades that
for speed); HC levels (>= 3) and the chunked / context streaming API are
outside this codec's scope.
"""
from __future__ import annotations

import os
import struct
import threading
import time

import torch

from .. import _native as N
from ..block._block import _buffer, _c_int

BLOCKSIZE_DEFAULT = 0
BLOCKSIZE_MAX64KB = 4
BLOCKSIZE_MAX256KB = 5
BLOCKSIZE_MAX1MB = 6
BLOCKSIZE_MAX4MB = 7

_MAGIC = 0x184D2204
_MAGIC_SKIPPABLE = 0x184D2A50
_BLOCK_SIZES = {4: 64 << 10, 5: 256 << 10, 6: 1 << 20, 7: 4 << 20}
_MIN_FH = 7        # lz4frame.c minFHSize
_BH = 4            # block header size
_UNCOMPRESSED = 0x80000000


def _err(fn: str, code: str) -> RuntimeError:
    return RuntimeError(f"{fn} failed with code: ERROR_{code}")


def _xxh32_dev(buf: bytes | memoryview | torch.Tensor, n: int | None = None, seed: int = 0) -> int:
    """XXH32 of a buffer: host bytes on this core; device bytes on a host
    core over pipelined PCIe copies."""
    if not isinstance(buf, torch.Tensor):
        return N.xxh32_host(buf, seed)
    return N.xxh32_of_device(buf, n if n is not None else buf.numel(), seed)


class _HashThread(threading.Thread):
    """The content checksum on a host core beside the device work."""

    def __init__(self, fn):
        super().__init__(daemon=True)
        self._fn = fn
        self.value = None
        self.error = None

    def run(self):
        try:
            self.value = self._fn()
        except BaseException as e:   # re-raised in the caller
            self.error = e

    def result(self) -> int:
        self.join()
        if self.error is not None:
            raise self.error
        return self.value


# ------------------------------------------------------------------ header
# Linked frames with at least _SPEC_MIN_BLOCKS blocks on average, in a call of
# fewer than _BATCH_SPEC_MAX_FRAMES linked frames, compress speculatively (a
# wavefront per block, lz4m_compress_linked_batch); otherwise one wavefront per
# frame, which is parallel over the frames
_SPEC_MIN_BLOCKS = 4
_BATCH_SPEC_MAX_FRAMES = 256


def _optimal_bsid(requested: int, size: int) -> int:
    """LZ4F_optimalBSID (lz4frame.c:351-363)."""
    proposed, max_size = 4, 64 << 10
    while requested > proposed:
        if size <= max_size:
            return proposed
        proposed += 1
        max_size <<= 2
    return requested


def _header(bsid: int, linked: bool, block_checksum: bool, content_size: int, content_checksum: bool) -> bytes:
    """LZ4F_compressBegin_usingCDict header (lz4frame.c:752-780)."""
    flg = (1 << 6) | ((0 if linked else 1) << 5) | (int(block_checksum) << 4) \
        | (int(content_size > 0) << 3) | (int(content_checksum) << 2)
    body = bytes([flg, (bsid & 7) << 4])
    if content_size:
        body += struct.pack("<Q", content_size)
    hc = (_xxh32_dev(body) >> 8) & 0xFF
    return struct.pack("<I", _MAGIC) + body + bytes([hc])


def _parse_header(mv: memoryview):
    """LZ4F_getFrameInfo -> LZ4F_headerSize + LZ4F_decodeHeader
    (lz4frame.c:1291-1380, 1387-1463).  Returns (info dict, header size)."""
    fn = "LZ4F_getFrameInfo"
    n = mv.nbytes
    if n < 5:
        raise _err(fn, "frameHeader_incomplete")
    magic = struct.unpack_from("<I", mv, 0)[0]
    if (magic & 0xFFFFFFF0) == _MAGIC_SKIPPABLE:
        if n < 8:
            raise _err(fn, "frameHeader_incomplete")
        return {"skippable": True, "frame_size": struct.unpack_from("<I", mv, 4)[0]}, 8
    if magic != _MAGIC:
        raise _err(fn, "frameType_unknown")
    flg = mv[4]
    hsize = _MIN_FH + (8 if flg & 0x08 else 0) + (4 if flg & 0x01 else 0)
    if n < hsize:
        raise _err(fn, "frameHeader_incomplete")
    if (flg >> 1) & 1:
        raise _err(fn, "reservedFlag_set")
    if (flg >> 6) & 3 != 1:
        raise _err(fn, "headerVersion_wrong")
    bd = mv[5]
    bsid = (bd >> 4) & 7
    if (bd >> 7) & 1:
        raise _err(fn, "reservedFlag_set")
    if bsid < 4:
        raise _err(fn, "maxBlockSize_invalid")
    if bd & 0x0F:
        raise _err(fn, "reservedFlag_set")
    hc = (_xxh32_dev(bytes(mv[4:hsize - 1])) >> 8) & 0xFF
    if hc != mv[hsize - 1]:
        raise _err(fn, "headerChecksum_invalid")
    info = {
        "skippable": False,
        "block_size_id": bsid,
        "block_size": _BLOCK_SIZES[bsid],
        "block_linked": not bool((flg >> 5) & 1),
        "block_checksum": bool((flg >> 4) & 1),
        "content_checksum": bool((flg >> 2) & 1),
        "content_size": struct.unpack_from("<Q", mv, 6)[0] if flg & 0x08 else 0,
        "dict_id": struct.unpack_from("<I", mv, hsize - 5)[0] if flg & 0x01 else 0,
    }
    return info, hsize


def get_frame_info(data):
    """get_frame_info(data) -- frame parameters of the frame at the start of
    data (_frame.c:640-824)."""
    mv = _buffer(data)
    info, _ = _parse_header(mv)
    if info["skippable"]:
        return {"block_size": 64 << 10, "block_size_id": BLOCKSIZE_MAX64KB, "block_linked": True,
                "content_checksum": False, "block_checksum": False, "skippable": True, "content_size": 0}
    return {k: info[k] for k in ("block_size", "block_size_id", "block_linked", "content_checksum",
                                  "block_checksum", "skippable", "content_size")}


# ---------------------------------------------------------------- compress
def compress(data, compression_level=0, block_size=0, content_checksum=False, block_checksum=False,
             block_linked=True, store_size=True, return_bytearray=False):
    """compress(data, compression_level=0, block_size=0, content_checksum=0,
    block_checksum=0, block_linked=True, store_size=True,
    return_bytearray=False) -- one LZ4 frame (_frame.c:112-259 ->
    LZ4F_compressFrame, lz4frame.c:420-515)."""
    src = _buffer(data, "data")
    level = _c_int(compression_level, "compression_level")
    bsid_req = _c_int(block_size, "block_size")
    dev = N.device()
    d_src = N.to_device(src, dev, pad=1)
    frame = _compress_frame(d_src, src.nbytes, compression_level=level, block_size=bsid_req,
                            content_checksum=content_checksum, block_checksum=block_checksum,
                            block_linked=block_linked, store_size=store_size, host_src=src)[0]
    return N.to_host_bytes(frame, frame.numel(), bool(return_bytearray))


def compress_device(d_src: torch.Tensor, n: int | None = None, *, compression_level=0, block_size=0,
                    content_checksum=False, block_checksum=False, block_linked=True, store_size=True,
                    parse="exact", stream=None) -> torch.Tensor:
    """Device-resident LZ4F_compressFrame: the frame of d_src[:n] as a uint8
    device tensor (no host round trip).

    parse="exact": blocks byte-identical to LZ4_compress_default, i.e. the
    frame is byte-identical to the reference's for independent blocks.
    parse="parallel": the parallel-parse compressor (valid blocks at the
    ratio of LZ4_compress_default, not byte-identical; BASELINE config 4).
    parse="hc" with compression_level >= 3: the hash-chain compressor at that
    level (valid blocks near LZ4F_compressFrame's size at the level, not
    byte-identical).  A linked frame's blocks, each with the 64 KiB of input
    before it as history, are compressed in one launch
    (lz4m_compress_hc_dict_batch).
    parse="optimal" with compression_level >= 3: the price-based optimal parse
    searching as that level (lz4m_compress_opt_batch; at level 9 within 1 % of
    the reference's level 12, not byte-identical).  Independent blocks only:
    with block_linked=True it raises NotImplementedError.

    The content checksum (one serial XXH32 stream over all of d_src) runs on
    a host core beside the block compression, over pipelined PCIe copies of
    d_src."""
    return _compress_frame(d_src, n, compression_level=compression_level, block_size=block_size,
                           content_checksum=content_checksum, block_checksum=block_checksum,
                           block_linked=block_linked, store_size=store_size, parse=parse, stream=stream)[0]


def _host_wait(stream) -> None:
    """Block until `stream` drains, with the GIL released (an event wait;
    tensor.item() waits holding the GIL, so a host hashing thread would sit
    idle for the whole device phase)."""
    ev = torch.cuda.Event()
    ev.record(stream)
    ev.synchronize()


class LinkedOptimalError(NotImplementedError, ValueError):
    """parse="optimal" asked for linked blocks: a combination that is not
    built (NotImplementedError) and, until it is, a bad value of ``parse`` for
    a linked frame (ValueError, what an unknown parse raises)."""


def resolve_parse(parse="exact", compression_level=0, block_linked=True) -> N.Parse:
    """The parse a device compression call's arguments ask for, as the
    description ``N.launch_blocks`` takes, or the call's argument error.  Its
    history names the block plan's array that goes with a linked frame's blocks
    ("link": one stream per frame, lz4frame.c:865-871; "hist": HC history; the
    parallel parse has none).  Pure: no data, no launch."""
    level = int(compression_level)
    if parse not in ("exact", "parallel", "hc", "optimal"):
        raise ValueError("parse must be 'exact', 'parallel', 'hc' or 'optimal'")
    if parse in ("hc", "optimal"):
        if level < 3:
            raise ValueError(f"parse='{parse}' needs compression_level >= 3 (levels 0-2 are the fast compressor)")
    elif level >= 3:
        raise NotImplementedError("LZ4 HC compression levels (>= 3) are outside the MI355X codec's scope")
    if parse == "optimal":
        if block_linked:
            raise LinkedOptimalError("parse='optimal' has no history: block_linked=True is not built "
                                     "(pass block_linked=False, or parse='hc' for linked blocks)")
        return N.Parse("opt", level=level)
    if parse == "hc":
        return N.Parse("hc", level=level, history="hist" if block_linked else "")
    accel = -level + 1 if level < 0 else 1                     # lz4frame.c:855
    if parse == "parallel":
        return N.Parse("table", N.PARSE_PARALLEL, accel, level)
    return N.Parse("table", N.TABLE_AUTO, accel, level, history="link" if block_linked else "")


def _plan_one(n, bsize, nb, history, dev) -> dict:
    """frames_plan_blocks' arrays for one frame of n bytes in nb blocks, built on the host (no plan kernel, no
    read-back); of link and hist, the one a linked frame's parse asks for (``history``)."""
    raw_off = torch.arange(nb, dtype=torch.int64, device=dev) * bsize
    raw_len = torch.full((nb,), bsize, dtype=torch.int32, device=dev)
    raw_len[-1] = n - (nb - 1) * bsize
    P = {"raw_off": raw_off, "raw_len": raw_len, "cap": raw_len - 1}   # lz4frame.c:835: dstCapacity = srcSize - 1
    if history == "link":                                      # one stream across the blocks
        P["link"] = torch.ones(nb, dtype=torch.int32, device=dev)
        P["link"][0] = 0
    elif history == "hist":                                    # the input before the block, at most 64 KiB
        P["hist"] = raw_off.clamp(max=65536).to(torch.int32)
    return P


def _compress_frame(d_src, n=None, *, compression_level=0, block_size=0, content_checksum=False,
                    block_checksum=False, block_linked=True, store_size=True, parse="exact", stream=None,
                    host_src=None):
    """compress_device, also returning the block records:
    (frame, {"data_off", "stored_len", "raw"}) with device tensors giving, per
    block, the payload position in the frame, its stored length and whether
    it is stored raw (None when the input is empty).  The pipeline of
    compress_batch for one frame: the plan and the header come from the host,
    the content hash runs on a host thread."""
    n = d_src.numel() if n is None else int(n)
    p = resolve_parse(parse, compression_level, block_linked)
    bsid = _optimal_bsid(int(block_size), n)
    if bsid == 0:
        bsid = BLOCKSIZE_MAX64KB                               # LZ4F_BLOCKSIZEID_DEFAULT
    if bsid not in _BLOCK_SIZES:
        raise RuntimeError("LZ4F_compressFrame failed with code: ERROR_maxBlockSize_invalid")
    bsize = _BLOCK_SIZES[bsid]
    linked = bool(block_linked) and n > bsize                  # lz4frame.c:441-442
    content_size = n if store_size else 0
    hdr = _header(bsid, linked, bool(block_checksum), content_size, bool(content_checksum))
    dev = d_src.device
    nb = (n + bsize - 1) // bsize
    total = 0
    body = None
    meta = None
    main = stream if stream is not None else torch.cuda.current_stream(dev)
    hthread = None
    if content_checksum:                                       # lz4frame.c:1042, 1170-1176
        if host_src is not None:     # the caller's bytes: hash them while the device compresses
            hthread = _HashThread(lambda: N.xxh32_host(host_src))
            hthread.start()
        else:                        # device bytes: streamed back and hashed while the device compresses
            ready = torch.cuda.Event()
            ready.record(main)       # before the compression is queued: the copies must not wait for it
            hthread = _HashThread(lambda: N.xxh32_of_device(d_src, n, wait_event=ready))
            hthread.start()
    if nb:
        P = _plan_one(n, bsize, nb, p.history if linked else "", dev)
        raw_off, raw_len = P["raw_off"], P["raw_len"]
        slot = N.compress_bound(bsize)
        cmp = torch.empty(nb * slot, dtype=torch.uint8, device=dev)
        cmp_off = torch.arange(nb, dtype=torch.int64, device=dev) * slot
        cmp_len = torch.empty(nb, dtype=torch.int32, device=dev)
        # max_len sizes workspaces: the block size, for the optimal parse the longest block
        _compress_blocks(d_src, P, cmp, cmp_off, cmp_len, p, linked, bsize > 65536,
                         min(bsize, n) if p.launcher == "opt" else bsize, 1, stream)
        rec_len = torch.empty(nb, dtype=torch.int32, device=dev)
        N.frame_block_sizes(raw_len, cmp_len, block_checksum, rec_len, nb, stream)
        frame_off = N.exclusive_scan(rec_len, stream=stream)
        if hthread is not None:   # wait with the GIL released: .item() waits holding it, stalling the hash thread
            _host_wait(main)
        total = int(frame_off[-1].item())
    tail = 4 + (4 if content_checksum else 0)
    out = torch.empty(len(hdr) + total + tail + 16, dtype=torch.uint8, device=dev)
    out[: len(hdr)] = torch.frombuffer(bytearray(hdr), dtype=torch.uint8).to(dev)
    if nb:
        body = out[len(hdr):]
        N.frame_emit(d_src, raw_off, raw_len, cmp, cmp_off, cmp_len, body, frame_off, block_checksum, nb, stream)
        del cmp
        stored = rec_len - 4 - (4 if block_checksum else 0)
        meta = {"data_off": frame_off[:nb] + len(hdr) + 4, "stored_len": stored,
                "raw": (cmp_len <= 0) | (cmp_len >= raw_len)}
    pos = len(hdr) + total
    out[pos: pos + 4] = 0                                      # endmark, lz4frame.c:1167
    if content_checksum:
        dig = hthread.result()
        out[pos + 4: pos + 8] = torch.frombuffer(bytearray(struct.pack("<I", dig)), dtype=torch.uint8).to(dev)
    return out[: pos + tail], meta


# -------------------------------------------------------------- decompress
def _scan_blocks(mv: memoryview, pos: int, info: dict):
    """Walk the block records the way LZ4F_decompress consumes them
    (lz4frame.c:1643-1701, 1926-1965).  Returns (records, end_state) where
    records = [(raw, data_pos, size, crc_pos)] and end_state is either
    ("end", bytes_read) or ("incomplete", hint) or ("error", code, index)."""
    n = mv.nbytes
    crc = 4 if info["block_checksum"] else 0
    maxb = info["block_size"]
    recs = []
    while True:
        if n - pos < _BH:
            return recs, ("incomplete", _BH - (n - pos))
        hdr = struct.unpack_from("<I", mv, pos)[0]
        pos += _BH
        if hdr == 0:                                           # endmark
            if info["content_checksum"]:
                if n - pos < 4:
                    return recs, ("incomplete_suffix", 4 - (n - pos), pos)
                return recs, ("end", pos + 4, pos)
            return recs, ("end", pos, None)
        size = hdr & 0x7FFFFFFF
        if size > maxb:
            return recs, ("error", "maxBlockSize_invalid", len(recs))
        raw = bool(hdr & _UNCOMPRESSED)
        avail = n - pos
        if raw:
            if avail < size + crc:
                got = min(avail, size)
                if avail <= size:
                    hint = (size - got) + crc + _BH
                else:
                    hint = crc - (avail - size) + _BH
                return recs, ("incomplete", hint if avail else _BH + size + crc)
        elif avail < size + crc:
            hint = (size + crc - avail) + crc + _BH if avail else _BH + size + crc
            return recs, ("incomplete", hint)
        recs.append((raw, pos, size, pos + size if crc else -1))
        pos += size + crc


def decompress(data, return_bytearray=False, return_bytes_read=False):
    """decompress(data, return_bytearray=False, return_bytes_read=False) --
    decode one full frame (_frame.c:1198-1258 -> __decompress 938-1193)."""
    mv = _buffer(data, "data")
    info, hsize = _parse_header(mv)
    if info["skippable"]:
        end = min(mv.nbytes, hsize + info["frame_size"])
        if mv.nbytes < hsize + info["frame_size"]:
            raise RuntimeError(f"Frame incomplete. LZ4F_decompress returned: {hsize + info['frame_size'] - mv.nbytes}")
        out = bytearray() if return_bytearray else b""
        return (out, end) if return_bytes_read else out
    recs, state = _scan_blocks(mv, hsize, info)
    if os.environ.get("LZ4M_FRAME_PIPELINE", "1") != "0":
        r = _decompress_pipelined(mv, info, recs, state, bool(return_bytearray))
        if r is not None:
            return (r, state[1]) if return_bytes_read else r
    dev = N.device()
    nb = len(recs)
    out_t, total, first_err = None, 0, None
    if nb:
        d_frame = N.to_device(mv, dev, pad=16)
        t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)   # noqa: E731
        args = (d_frame, info, nb, t([r[1] for r in recs], torch.int64), t([r[2] for r in recs], torch.int32),
                t([r[0] for r in recs], torch.bool), t([r[3] for r in recs], torch.int64))
        out_t, total, first_err, _ = _decode_records(*args)
    _frame_errors(first_err, state, info, total)
    if info["content_checksum"]:   # on the copy the caller gets, hashed while it is staged (lz4frame.c:1850, 1959-1964)
        out, got = N.to_host_bytes(out_t, total, bool(return_bytearray), hash_seed=0)
        if got != struct.unpack_from("<I", mv, state[2])[0]:
            raise _err("LZ4F_decompress", "contentChecksum_invalid")
    else:
        out = N.to_host_bytes(out_t, total, bool(return_bytearray))
    return (out, state[1]) if return_bytes_read else out


class _FeedHash(threading.Thread):
    """The content XXH32 on a host core, over host ranges handed to it in
    order (put(ptr, n); put(None) ends it)."""

    def __init__(self):
        super().__init__(daemon=True)
        import queue
        self.q = queue.SimpleQueue()
        self.st = N.HostXXH32(0)
        self.error = None

    def put(self, ptr, n=0):
        self.q.put(None if ptr is None else (ptr, n))

    def run(self):
        try:
            while True:
                item = self.q.get()
                if item is None:
                    return
                self.st.update_ptr(*item)
        except BaseException as e:   # re-raised in the caller
            self.error = e

    def digest(self) -> int:
        self.put(None)
        self.join()
        if self.error is not None:
            raise self.error
        return self.st.digest()


def _decompress_pipelined(mv, info, recs, state, as_bytearray):
    """``decompress`` of a large well-formed frame of independent compressed
    blocks with a stored content size, as one pipeline: the frame goes to the
    device in 64 MiB chunks, the blocks decode in three block-ordered launches
    as their bytes land, the output comes back in 64 MiB chunks as
    their launch ends -- straight into the result bytes -- and a host core
    hashes the result behind the copies (the content checksum, lz4frame.c:1850,
    one serial stream: the bound).  The stages that ran one after another
    (upload, decode, download + hash) overlap.

    Every block but the last is taken to decode to the full block size (what
    LZ4F_compressFrame writes), so the slots are the output; this, the
    statuses and the block checksums are checked at the end, and on any
    mismatch this returns None and the caller decodes the frame the
    sequential way (which raises the reference's exact error).  Also None
    when the frame does not qualify.

    A launch takes about one block's decode time whatever its size (one
    wavefront per block; a 4 MiB block ~51 ms, profiles/r05/r05y), so the
    launches are few and growing -- 1/16, 3/16, 12/16 of the blocks -- and
    the first two run on two streams side by side: the first output is ready
    one block-decode after 1/16 of the frame has landed, and the rest stays
    ahead of the hash."""
    nb = len(recs)
    maxb = info["block_size"]
    total = info["content_size"]
    n = mv.nbytes
    if (state[0] != "end" or info["block_linked"] or nb < 32 or n < N._BIG
            or not total or not ((nb - 1) * maxb < total <= nb * maxb)
            or any(r[0] for r in recs)):
        return None
    dev = N.device()
    main = torch.cuda.current_stream(dev)
    up = torch.cuda.Stream(dev, priority=-1)
    down = torch.cuda.Stream(dev, priority=-1)
    side = torch.cuda.Stream(dev)          # the second decode stream
    crc = info["block_checksum"]
    c_off = torch.tensor([r[1] for r in recs], dtype=torch.int64, device=dev)
    c_len = torch.tensor([r[2] for r in recs], dtype=torch.int32, device=dev)
    status = torch.empty(nb, dtype=torch.int32, device=dev)
    sums = torch.empty(nb, dtype=torch.int32, device=dev) if crc else None
    slots, slot_off, caps = _decode_slots(nb, maxb, dev)
    d_frame = torch.empty(n + 16, dtype=torch.uint8, device=dev)
    d_frame[n:].zero_()
    up.wait_stream(main)   # (after the allocations: their memory may be free only in main's order)
    side.wait_stream(main)
    C = N._CHUNK
    thr = N._copy_threads()
    src = N.host_addr(mv)
    out, dst = N._new_host_buffer(total, as_bytearray)
    hasher = _FeedHash() if info["content_checksum"] else None
    if hasher is not None:
        hasher.start()
    # spans: block-ordered decode launches; span k needs the frame up to ends[k]
    bounds = [0, nb // 16, nb // 4, nb]
    K = len(bounds) - 1
    ends = [recs[bounds[k + 1] - 1][1] + recs[bounds[k + 1] - 1][2] + (4 if crc else 0) for k in range(K)]
    span_ev = [None] * K
    trace = [] if os.environ.get("LZ4M_PIPE_TRACE") else None
    t0 = time.perf_counter()
    fills = [(lo, min(n, lo + C)) for lo in range(0, n, C)]
    drains = [(lo, min(total, lo + C)) for lo in range(0, total, C)]
    # the span whose launch writes the last byte of each drain chunk
    need = [next(k for k in range(K) if (b - 1) // maxb < bounds[k + 1]) for _, b in drains]
    upb, downb = N._pinned_pair(C), N._pinned_pair(C)
    up_ev, down_ev = [None, None], [torch.cuda.Event(), torch.cuda.Event()]
    launched = 0
    fi = di = dd = 0   # next fill, next drain to issue, next drain to finish
    done = False
    try:
        while dd < len(drains):
            # a download is queued only once its launch is done: a copy queued
            # behind an event holds up the uploads (r05ac: the second launch
            # waited for the first launch's end)
            while di < len(drains) and di - dd < 2 and need[di] < launched and span_ev[need[di]].query():
                lo, hi = drains[di]
                with torch.cuda.stream(down):
                    downb[di & 1][: hi - lo].copy_(slots[lo:hi], non_blocking=True)
                    down_ev[di & 1].record(down)
                di += 1
            if dd < di and (fi == len(fills) or down_ev[dd & 1].query()):
                lo, hi = drains[dd]
                down_ev[dd & 1].synchronize()
                N.lib().lz4m_host_copy(dst + lo, downb[dd & 1].data_ptr(), hi - lo, thr, None)
                if hasher is not None:
                    hasher.put(dst + lo, hi - lo)
                if trace is not None:
                    trace.append(("drain", dd, time.perf_counter() - t0))
                dd += 1
                continue
            if fi < len(fills):   # upload the next frame chunk, launch the spans it completes
                lo, hi = fills[fi]
                b = upb[fi & 1]
                if up_ev[fi & 1] is not None:
                    up_ev[fi & 1].synchronize()
                N.lib().lz4m_host_copy(b.data_ptr(), src + lo, hi - lo, thr, None)
                with torch.cuda.stream(up):
                    d_frame[lo:hi].copy_(b[: hi - lo], non_blocking=True)
                    up_ev[fi & 1] = torch.cuda.Event()
                    up_ev[fi & 1].record(up)
                fi += 1
                while launched < K and ends[launched] <= hi:
                    k = launched
                    st = side if k == 1 else main
                    st.wait_event(up_ev[(fi - 1) & 1])
                    a, z = bounds[k], bounds[k + 1]
                    with torch.cuda.stream(st):
                        if crc:
                            N.launch_xxh32_batch(d_frame, c_off[a:z], c_len[a:z].to(torch.int64), 0, sums[a:z], z - a,
                                                 stream=st)
                        N.launch_decompress(d_frame, c_off[a:z], c_len[a:z], slots, slot_off[a:z], caps[a:z],
                                            status[a:z], z - a, stream=st)
                        span_ev[k] = torch.cuda.Event(enable_timing=trace is not None)
                        span_ev[k].record(st)
                    if trace is not None:
                        trace.append(("launch", k, time.perf_counter() - t0))
                    launched += 1
                continue
            if dd == di:   # everything uploaded and launched: wait for the next download's launch
                span_ev[need[di]].synchronize()
        done = True
    finally:
        if hasher is not None and not done:
            # the thread may still be hashing `out`, freed once the exception
            # leaves this function: it must have ended first
            hasher.put(None)
            hasher.join()
        # (on an error too: no copy or launch may still use the buffers freed on return)
        for e in up_ev + down_ev + span_ev:
            if e is not None:
                e.synchronize()
        N._pinned_release(C, upb)
        N._pinned_release(C, downb)
    got = hasher.digest() if hasher is not None else None
    main.wait_stream(side)
    if trace is not None:
        import sys
        trace.append(("hash", 0, time.perf_counter() - t0))
        print("[lz4m] pipelined frame decode: " + " ".join(f"{a}{b}@{c * 1e3:.1f}" for a, b, c in trace
                                                          if a != "drain" or b % 16 == 0 or b == len(drains) - 1),
              file=sys.stderr, flush=True)
    ok = (status[: nb - 1] == maxb).all() & (status[nb - 1] == total - (nb - 1) * maxb)
    if crc:
        crc_pos = torch.tensor([r[3] for r in recs], dtype=torch.int64, device=dev)
        ok = ok & ~_crc_mismatch(d_frame, sums, crc_pos).any()
    if not bool(ok):
        return None
    if info["content_checksum"] and got != struct.unpack_from("<I", mv, state[2])[0]:
        raise _err("LZ4F_decompress", "contentChecksum_invalid")
    return out


def decompress_device(d_frame: torch.Tensor, n: int | None = None, stream=None) -> torch.Tensor:
    """Device-resident LZ4F_decompress: decode the frame in d_frame[:n] (a
    uint8 device tensor) into a new uint8 device tensor, with no host copy of
    the data (BASELINE config 4).  The header is parsed on
    the host from its first bytes; the block records are walked on the device
    (lz4m_frame_scan); independent blocks decode in one batched launch, linked
    ones on the chain kernel; block checksums are verified on the device, the
    content checksum on a host core over pipelined PCIe copies of the output.
    A malformed or truncated frame raises exactly what ``decompress`` raises
    for the same bytes."""
    n = d_frame.numel() if n is None else int(n)
    dev = d_frame.device
    head = bytes(d_frame[: min(n, 19)].cpu().numpy().tobytes())
    try:
        info, hsize = _parse_header(memoryview(head))
    except RuntimeError:
        if n <= 19:
            raise
        info, hsize = None, 0
    if info is None or info["skippable"] or n <= hsize:
        return _via_host_path(d_frame, n)   # errors and skippable frames
    max_rec = n // 64 + 1024
    rec_pos = torch.empty(max_rec, dtype=torch.int64, device=dev)
    rec_len = torch.empty(max_rec, dtype=torch.int32, device=dev)
    rec_raw = torch.empty(max_rec, dtype=torch.uint8, device=dev)
    # (the records' checksum positions come from the scan too; nothing reads them without block checksums)
    rec_crc = torch.empty(max_rec, dtype=torch.int64, device=dev) if info["block_checksum"] else None
    res = torch.zeros(4, dtype=torch.int64, device=dev)
    N.frame_scan(d_frame, n, hsize, info["block_checksum"], info["content_checksum"], info["block_size"], max_rec,
                 rec_pos, rec_len, rec_raw, rec_crc, res, stream)
    nb, st, _end, cpos = (int(v) for v in res.cpu().tolist())
    if st != 0:   # malformed / truncated (or > max_rec records)
        return _via_host_path(d_frame, n)
    out_t, total, first_err, got = None, 0, None, None
    if nb:
        out_t, total, first_err, got = _decode_records(d_frame, info, nb, rec_pos[:nb], rec_len[:nb],
                                                       rec_raw[:nb].to(torch.bool),
                                                       None if rec_crc is None else rec_crc[:nb],
                                                       follow_hash=bool(info["content_checksum"]))
    _frame_errors(first_err, ("end", _end, cpos if cpos >= 0 else None), info, total)
    if info["content_checksum"]:
        want = int(_le32_at(d_frame, torch.tensor([cpos], dtype=torch.int64, device=dev)).item()) & 0xFFFFFFFF
        if got is None:
            got = _xxh32_dev(out_t, total) if total else _xxh32_dev(b"")
        if got != want:
            raise _err("LZ4F_decompress", "contentChecksum_invalid")
    if not total:
        return torch.empty(0, dtype=torch.uint8, device=dev)
    return out_t[:total]


def _via_host_path(d_frame, n):
    """decompress_device by ``decompress`` of a host copy of the frame: the host path's exact result or error."""
    return N.to_device(decompress(d_frame[:n].cpu().numpy().tobytes()), d_frame.device)


def _le32_at(d_buf, pos):
    """LE32 values at device positions `pos` of d_buf (int64 tensor)."""
    idx = pos[:, None] + torch.arange(4, dtype=torch.int64, device=pos.device)
    b = d_buf[idx].to(torch.int64)
    return b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)


def _frame_errors(first_err, state, info, total):
    """The error order of __decompress / LZ4F_decompress (lz4frame.c:1819,
    1844-1847, 1927): first failing block, then a structural error, then
    truncation, then the content size."""
    dec = "LZ4F_decompress"
    if first_err is not None:
        raise _err(dec, first_err[1])
    if state[0] == "error":
        raise _err(dec, state[1])
    if state[0] == "incomplete":
        raise RuntimeError(f"Frame incomplete. LZ4F_decompress returned: {state[1]}")
    if info["content_size"] and total != info["content_size"]:
        raise _err(dec, "frameSize_wrong")                     # lz4frame.c:1927
    if state[0] == "incomplete_suffix":
        raise RuntimeError(f"Frame incomplete. LZ4F_decompress returned: {state[1]}")


# block-ordered decode launches the content hash follows (decompress_device).
# A launch takes about one block's decode time whatever its size (4 MiB
# blocks: ~51 ms, profiles/r05/r05y): 16 launches (826 ms) fell behind the
# hash; 2, 4 and 8 launches measured 674-682 ms (r05y, r05ab)
_FOLLOW_CHUNKS = 4


def _decode_slots(nb, maxb, dev):
    """(slots, slot_off, caps): a decode slot of the frame's block size per block (lz4frame.c:1844-1847)."""
    return (torch.empty(nb * maxb + 16, dtype=torch.uint8, device=dev),
            torch.arange(nb, dtype=torch.int64, device=dev) * maxb,
            torch.full((nb,), maxb, dtype=torch.int32, device=dev))


def _crc_mismatch(d_frame, sums, crc_pos):
    """Mask of the blocks whose XXH32 (``sums``, int32) is not the LE32 at crc_pos[i] of the frame."""
    return (sums.to(torch.int64) & 0xFFFFFFFF) != _le32_at(d_frame, crc_pos)


def _block_crc_bad(d_frame, info, c_off, c_len, crc_pos):
    """_crc_mismatch of every block (lz4frame.c:1819: verified first per block); None without block checksums."""
    if not info["block_checksum"]:
        return None
    sums = torch.empty(c_off.numel(), dtype=torch.int32, device=d_frame.device)
    N.launch_xxh32_batch(d_frame, c_off, c_len.to(torch.int64), 0, sums, c_off.numel())
    return _crc_mismatch(d_frame, sums, crc_pos)


def _first_error(bad_dec, crc_bad):
    """(index, code) of the first block that failed to decode (mask bad_dec)
    or whose checksum differs (mask crc_bad or None); None when all are good."""
    bad = bad_dec if crc_bad is None else (bad_dec | crc_bad)
    if not bool(bad.any()):
        return None
    i = int(torch.nonzero(bad).flatten()[0])
    return i, "blockChecksum_invalid" if crc_bad is not None and bool(crc_bad[i]) else "decompressionFailed"


def _decode_records(d_frame, info, nb, c_off, c_len, raw_mask, crc_pos, follow_hash=False):
    """Decode nb block records of a frame in device memory: payload at
    c_off[i] (int64), stored size c_len[i] (int32), raw_mask[i] = stored
    uncompressed, crc_pos[i] = position of its LE32 block checksum (unused,
    and may be None, without block checksums).
    Returns (out tensor, total decoded bytes, first error or None, the
    content XXH32 of the output or None when the caller must hash it).

    ``follow_hash`` (independent blocks, no stored ones): the blocks decode
    in _FOLLOW_CHUNKS launches in block order, and a host thread hashes each
    launch's output as soon as it is done (lz4frame.c:1849-1850 hashes the
    output in order), reading it from the decode slots on the assumption
    that every block but the last decodes to the full block size (what
    LZ4F_compressFrame writes), so the slots are the output.  The assumption
    is checked once the decode is done; if it fails, the hash is discarded
    and the output gathered and hashed as before."""
    if follow_hash:
        r = _decode_records_follow(d_frame, info, nb, c_off, c_len, raw_mask, crc_pos)
        if r is not None:
            return r
    dev = d_frame.device
    maxb = info["block_size"]
    status = torch.empty(nb, dtype=torch.int32, device=dev)
    crc_bad = _block_crc_bad(d_frame, info, c_off, c_len, crc_pos)
    slots, slot_off, caps = _decode_slots(nb, maxb, dev)
    linked = info["block_linked"] and nb > 1 and not bool(raw_mask.all())
    if linked:
        _decode_linked(d_frame, c_off, c_len, raw_mask, slots, slot_off, caps, status, maxb)
    else:
        # raw blocks are handed to the decoder with length 0 (immediate
        # reject, no work); they are gathered from the frame below
        dec_len = torch.where(raw_mask, torch.zeros_like(c_len), c_len)
        N.launch_decompress(d_frame, c_off, dec_len, slots, slot_off, caps, status, nb)
    sizes = torch.where(raw_mask, c_len, status) if not linked else status
    err = _first_error((~raw_mask) & (status < 0), crc_bad)
    if err is not None:
        return None, 0, err, None
    if linked:
        return slots, int(sizes.to(torch.int64).sum()), None, None
    # no stored block and every block but the last full (what LZ4F_compressFrame
    # writes): the slots already are the output, no gather (one read-back)
    chk = torch.stack([(~raw_mask).all().to(torch.int64), (status[: nb - 1] == maxb).all().to(torch.int64),
                       status[nb - 1].to(torch.int64)]).cpu()
    if int(chk[0]) and int(chk[1]):
        return slots, (nb - 1) * maxb + int(chk[2]), None, None
    lens = sizes.to(torch.int32)
    offs = N.exclusive_scan(lens)
    total = int(offs[-1].item())
    out_t = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    sel_c = torch.nonzero(~raw_mask).flatten()
    sel_r = torch.nonzero(raw_mask).flatten()
    if sel_c.numel():                                          # compressed blocks from the slots
        N.gather(slots, slot_off[sel_c], lens[sel_c], out_t, offs[sel_c], sel_c.numel())
    if sel_r.numel():                                          # raw blocks straight from the frame
        N.gather(d_frame, c_off[sel_r], lens[sel_r], out_t, offs[sel_r], sel_r.numel())
    return out_t, total, None, None


def _decode_records_follow(d_frame, info, nb, c_off, c_len, raw_mask, crc_pos):
    """_decode_records(follow_hash=True) for frames it applies to, else None."""
    if info["block_linked"] or nb < 2 * _FOLLOW_CHUNKS or bool(raw_mask.any()):
        return None
    dev = d_frame.device
    maxb = info["block_size"]
    status = torch.empty(nb, dtype=torch.int32, device=dev)
    crc_bad = _block_crc_bad(d_frame, info, c_off, c_len, crc_pos)
    slots, slot_off, caps = _decode_slots(nb, maxb, dev)
    bounds = [nb * k // _FOLLOW_CHUNKS for k in range(_FOLLOW_CHUNKS + 1)]
    spans = []
    for k in range(_FOLLOW_CHUNKS):
        lo, hi = bounds[k], bounds[k + 1]
        N.launch_decompress(d_frame, c_off[lo:hi], c_len[lo:hi], slots, slot_off[lo:hi], caps[lo:hi],
                            status[lo:hi], hi - lo)
        ev = torch.cuda.Event()
        ev.record()
        # full blocks only: the last block's size is known after the decode
        spans.append((lo * maxb, min(hi, nb - 1) * maxb, ev))
    hasher = _HashThread(lambda: N.xxh32_of_device_spans(slots, spans))
    hasher.start()
    try:
        # wait for the decode on the last launch's event, which releases the
        # GIL (a tensor read-back waits holding it, and the hash thread needs
        # it between chunks: r05p measured no overlap that way)
        spans[-1][2].synchronize()
        err = _first_error(status < 0, crc_bad)
        if err is not None:
            return None, 0, err, None
        st = status.cpu()
        full = bool((st[: nb - 1] == maxb).all())
    finally:
        hasher.join()
    if not full:
        return None
    total = (nb - 1) * maxb + int(st[nb - 1])
    state = hasher.result()
    state = N.xxh32_of_device_spans(slots, [((nb - 1) * maxb, total, None)], state=state)
    return slots, total, None, state.digest()


def _decode_linked(d_frame, c_off, c_len, raw_mask, out, slot_off, caps, status, maxb):
    """Linked blocks: each block may reference the previous output
    (LZ4F_updateDict, lz4frame.c:1853-1856: LZ4_decompress_safe_usingDict
    with the last <= 64 KiB decoded), contiguously into `out`.

    Speculatively in rounds: every block decodes at once with the previous
    round's output as its dictionary (two buffers), until a round changes no
    byte and no status.  At that fixed point block k was decoded with the
    true output of block k-1 and, by induction from block 0 (no dictionary),
    every block equals the serial chain's.  A round is one launch of the
    one-wavefront-per-block decoder with the other buffer as dictionary
    (lz4m_decompress_batch_prefix; LZ4M_LINKED_DECODE=dict: the lane-per-
    block dictionary kernel).  This needs every block but the last to decode
    to exactly the block size (what LZ4F_compressFrame and the lz4 tool
    write); otherwise, or with LZ4M_LINKED_DECODE=serial, blocks decode in
    order on one wavefront (lz4m_decompress_chain)."""
    nb = c_off.numel()
    mode = os.environ.get("LZ4M_LINKED_DECODE", "")
    if nb <= 2 or mode == "serial":
        N.launch_decompress_chain(d_frame, c_off, c_len, raw_mask, out, status, nb, maxb)
        return
    dev = d_frame.device
    span = nb * maxb
    dec_len = torch.where(raw_mask, torch.zeros_like(c_len), c_len)
    dlen = torch.clamp(slot_off, max=65536)
    dict_off = slot_off - dlen
    dlen = dlen.to(torch.int32)
    # both buffers start zeroed: the decoder leaves a slot's bytes past the
    # block's decoded length untouched, so a short last block (or a failing
    # one) must see equal bytes there in both or the fixed point never shows
    out[:span].zero_()
    bufs = [out, torch.zeros_like(out)]
    sts = [torch.empty(nb, dtype=torch.int32, device=dev), torch.empty(nb, dtype=torch.int32, device=dev)]
    sel_r = torch.nonzero(raw_mask).flatten()
    for b in bufs:                                             # stored blocks: their bytes, every round
        if sel_r.numel():
            N.gather(d_frame, c_off[sel_r], c_len[sel_r], b, slot_off[sel_r], sel_r.numel())
    cur = 0
    for r in range(nb + 1):
        prev = cur ^ 1
        if mode == "dict":
            N.launch_decompress(d_frame, c_off, dec_len, bufs[cur], slot_off, caps, sts[cur], nb,
                                dict_buf=bufs[prev], dict_off=dict_off, dict_len=dlen)
        else:
            N.launch_decompress_prefix(d_frame, c_off, dec_len, bufs[cur], slot_off, caps, bufs[prev], dlen,
                                       sts[cur], nb)
        sts[cur] = torch.where(raw_mask, c_len, sts[cur])
        if r > 0 and torch.equal(sts[cur], sts[prev]) and torch.equal(bufs[cur][:span], bufs[prev][:span]):
            break
        cur = prev
    if bufs[cur] is not out:
        out[:span].copy_(bufs[cur][:span])
    _linked_status(d_frame, c_off, c_len, raw_mask, out, status, nb, maxb, sts[cur])


def _linked_status(d_frame, c_off, c_len, raw_mask, out, status, nb, maxb, st):
    """Accept the speculative result unless a block before the first failing
    one decoded short of the block size (then the blocks' positions differ
    from the slots: the serial chain decodes the frame instead)."""
    bad = st < 0
    upto = int(torch.nonzero(bad).flatten()[0]) if bool(bad.any()) else nb - 1
    if upto > 0 and not bool((st[:upto] == maxb).all()):       # a short block mid-frame: positions differ
        N.launch_decompress_chain(d_frame, c_off, c_len, raw_mask, out, status, nb, maxb)
        return
    status.copy_(st)


# ------------------------------------------------------------ batched frames
# Many frames per call.  What is serial inside a frame
# (its header, the walk over its block records, a linked chain, its content
# hash) runs on one lane or one wavefront per frame, the frames side by side;
# the blocks of all frames share the block-batched launches.  The number of
# launches and host synchronisations of a call does not depend on the number
# of frames: the host reads back totals (block count, buffer sizes) only.


def _on(stream):
    import contextlib
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


def _spans(buf, off, length, what):
    """(int64 offsets, int64 lengths, sum of the lengths) of n spans of a uint8 device tensor, checked to lie
    inside it (one read-back)."""
    if buf.dtype != torch.uint8 or not buf.is_cuda:
        raise TypeError(f"{what} must be a uint8 device tensor")
    if off.numel() != length.numel():
        raise ValueError(f"{what}: offsets and lengths differ in count")
    off = off.to(device=buf.device, dtype=torch.int64).contiguous().view(-1)
    length = length.to(device=buf.device, dtype=torch.int64).contiguous().view(-1)
    if off.numel() == 0:
        return off, length, 0
    lo, neg, hi, total = torch.stack([off.min(), length.min(), (off + length).max(), length.sum()]).tolist()
    if lo < 0 or neg < 0 or hi > buf.numel():
        raise ValueError(f"{what}: a span reaches outside the buffer")
    return off, length, total


def compress_batch(src, src_off, src_len, *, compression_level=0, block_size=0, content_checksum=False,
                   block_checksum=False, block_linked=True, store_size=True, parse="exact", stream=None):
    """compress_device for n inputs in one call: input i is
    src[src_off[i] : src_off[i] + src_len[i]] of a uint8 device tensor.
    Returns (frames, frame_off, frame_len): frame i is
    frames[frame_off[i] : frame_off[i] + frame_len[i]] (int64 device tensors;
    the frames lie back to back).  Frame i holds the bytes of
    ``compress_device(input i, same options)`` for parse="exact" and
    parse="hc" and parse="optimal" (independent blocks only: block_linked=True
    raises NotImplementedError); parse="parallel" gives valid frames of the
    parallel parse.

    The blocks of all frames are compressed together: those of linked frames
    (block_linked and an input above one block) as one stream per frame
    (lz4m_compress_linked_batch; parse="hc": lz4m_compress_hc_dict_batch with
    each block's history), all others as independent blocks -- a batch whose
    inputs straddle the block size uses both.  Content checksums are hashed
    on the device, four lanes per frame (lz4m_xxh32_batch): a very large frame
    in a batch hashes serially; that is what the single-frame calls are for."""
    p = resolve_parse(parse, compression_level, block_linked)
    req = max(-1, min(int(block_size), 8))   # beyond 7 it is no block size whatever the input's length
    with _on(stream):
        off, ln, src_total = _spans(src, src_off, src_len, "src")
        dev = src.device
        n = off.numel()
        if n == 0:
            e = torch.empty(0, dtype=torch.int64, device=dev)
            return torch.empty(0, dtype=torch.uint8, device=dev), e, e.clone()
        bsid, nblocks, linked = N.frames_plan(ln, n, req, block_linked)
        base = N.exclusive_scan(nblocks)
        nb, bad, top, n_linked = torch.stack([base[-1], (bsid < 0).sum(), bsid.max(), linked.sum()]).tolist()
        if bad:
            raise RuntimeError("LZ4F_compressFrame failed with code: ERROR_maxBlockSize_invalid")
        hashes = None
        if content_checksum:                                   # lz4frame.c:1042, 1170-1176
            hashes = torch.empty(n, dtype=torch.int32, device=dev)
            N.launch_xxh32_batch(src, off, ln, 0, hashes, n)
        if nb:
            P = N.frames_plan_blocks(off, ln, bsid, linked, base, n, nb)
            cmp_off = N.exclusive_scan(P["slot_len"])
            cmp = torch.empty(src_total + src_total // 255 + 17 * nb + 64, dtype=torch.uint8, device=dev)
            cmp_len = torch.zeros(nb, dtype=torch.int32, device=dev)
            # the per-block masks, where the parse splits by them and the plan is not uniform
            owner = P["owner"]
            in_linked = linked[owner] != 0 if n_linked and p.history else False
            big = bsid[owner] > BLOCKSIZE_MAX64KB if top > BLOCKSIZE_MAX64KB and p.table == N.PARSE_PARALLEL else False
            _compress_blocks(src, P, cmp, cmp_off[:nb].contiguous(), cmp_len, p, in_linked, big, _BLOCK_SIZES[top],
                             n_linked)
            rec_len = torch.empty(nb, dtype=torch.int32, device=dev)
            N.frame_block_sizes(P["raw_len"], cmp_len, block_checksum, rec_len, nb)
            rec_off = N.exclusive_scan(rec_len)
        else:
            rec_off = torch.zeros(1, dtype=torch.int64, device=dev)
        hsize, fsize = N.frames_sizes(rec_off, base, ln, store_size, content_checksum, n)
        fend = torch.cumsum(fsize, 0)
        frame_off = fend - fsize
        total = int(fend[-1])
        frames = torch.empty(total + 16, dtype=torch.uint8, device=dev)
        if nb:
            shift = frame_off + hsize - rec_off[base[:-1]]     # frame position of a frame's first record
            blk_off = rec_off[:nb] + shift[P["owner"]]
            N.frame_emit(src, P["raw_off"], P["raw_len"], cmp, cmp_off, cmp_len, frames, blk_off, block_checksum, nb)
        N.frames_emit(frames, frame_off, fsize, bsid, linked, ln, store_size, block_checksum, content_checksum,
                      hashes, n)
        return frames[:total], frame_off, fsize


def _compress_blocks(src, P, cmp, cmp_off, cmp_len, p, linked, big, max_len, n_linked, stream=None):
    """The block stage of every frame compression: the planned blocks (P: frames_plan_blocks' arrays or
    _plan_one's) into their slots of `cmp` with the parse ``p``, in at most two launches picked per block.
    ``linked``: the block's frame is linked; ``big``: its blocks are above 64 KiB -- a bool where the host knows
    one answer for all blocks (a single frame; a batch whose plan found none: no read-back), else a mask (one
    read-back each way).  ``max_len`` bounds the longest block; ``n_linked`` counts the linked frames."""
    if p.launcher == "table" and p.table == N.PARSE_PARALLEL:  # by block size: the large-block launch above 64 KiB
        groups = [(p, big, False), (p._replace(table=N.PARSE_PARALLEL_LARGE), big, True)]
    elif p.history:                                            # by linking: P[p.history] goes with a linked frame's blocks
        groups = [(p._replace(history=""), linked, False), (p, linked, True)]
    else:
        groups = [(p, False, False)]
    arrays = (P["raw_off"], P["raw_len"], cmp_off, P["cap"], P.get(p.history))
    nb = cmp_len.numel()
    for q, mask, want in groups:
        sel = None                                             # the blocks where the mask says `want`; None: all
        if isinstance(mask, bool):
            if mask != want:
                continue
        else:
            sel = torch.nonzero(mask if want else ~mask).flatten()
            if sel.numel() == 0:
                continue
            if sel.numel() == nb:
                sel = None
        o, ln, co, cap, extra = arrays if sel is None else (a if a is None else a[sel] for a in arrays)
        m = nb if sel is None else sel.numel()
        out = cmp_len if sel is None else torch.empty(m, dtype=torch.int32, device=cmp_len.device)
        # few linked frames of at least _SPEC_MIN_BLOCKS blocks on average: speculatively, a wavefront per block
        spec = n_linked < _BATCH_SPEC_MAX_FRAMES and m >= _SPEC_MIN_BLOCKS * n_linked
        N.launch_blocks(q, src, o, ln, cmp, co, cap, out, m, extra=extra if q.history else None, max_len=max_len,
                        speculative=spec, stream=stream)
        if sel is not None:
            cmp_len[sel] = out


def decompress_batch(frames, frame_off, frame_len, *, stream=None, direct: bool = False):
    """decompress_device for n frames in one call: frame i is the
    frame_len[i] bytes at frames[frame_off[i]] of a uint8 device tensor
    (bytes after a frame's end are allowed).  Returns (out, out_off, out_len,
    status, bytes_read), device tensors: status[i] == 0 exactly when
    ``decompress`` of those bytes succeeds; then
    out[out_off[i] : out_off[i] + out_len[i]] is its result and bytes_read[i]
    the bytes it consumed.  A skippable frame has status 0 and length 0.  A
    non-zero status is a code of include/lz4m.h (LZ4M_FRAME_*): a malformed or
    truncated frame, a block that does not decode, a block or content
    checksum mismatch, a stored content size that differs; that frame's output
    span is then unspecified.  No frame's failure changes another frame.

    Two passes find the blocks (lz4m_frames_scan, lz4m_frames_records); the
    blocks of independent frames decode in one launch into slots of their
    frame's block size, linked frames one wavefront per frame
    (lz4m_decompress_chains); one gather packs the blocks of every frame
    back to back (a block may decode short of the block size) and takes stored
    blocks from the frame.  Checksums are verified on the device; the content
    hash is four lanes per frame.

    ``direct=True``: the compressed blocks of frames that are not chains
    (chains: linked frames of more than one block) are sized first
    (lz4m_decompressed_size_batch) and decode straight into ``out`` at their
    final positions with their size as capacity: no slots for these frames
    and no second copy of their bytes.  Chains keep the slots, for their
    frames only (their kernel gives every block the frame's block size as
    capacity, and its wild stores would reach the next frame's bytes in a
    packed buffer).  For frames written by any compressor of this package or
    the reference the five tensors are those of ``direct=False``.  One
    difference: a block that decodes only with slack (its last match starts
    within 12 bytes of the block's end or ends within 5; no conformant
    compressor writes one) fails at its exact size, so a frame holding one
    has status LZ4M_FRAME_BLOCK_FAILED here where ``direct=False`` reports
    what the rest of the frame gives (0 without a content checksum)."""
    with _on(stream):
        off, ln, _ = _spans(frames, frame_off, frame_len, "frames")
        dev = frames.device
        n = off.numel()
        if n == 0:
            e64 = lambda: torch.empty(0, dtype=torch.int64, device=dev)   # noqa: E731
            return (torch.empty(0, dtype=torch.uint8, device=dev), e64(), e64(),
                    torch.empty(0, dtype=torch.int32, device=dev), e64())
        S = N.frames_scan(frames, off, ln, n)
        base = N.exclusive_scan(S["nblocks"])
        flags = S["flags"]
        maxb = torch.ones_like(S["content_size"]) << (8 + 2 * S["bsid"].to(torch.int64))
        fcap = S["nblocks"].to(torch.int64) * maxb
        chain = ((flags & N.FRAME_LINKED) != 0) & (S["nblocks"] > 1)   # lz4frame.c:1853-1856
        if direct:   # slots for the chains only
            fcap = torch.where(chain, fcap, torch.zeros_like(fcap))
        slot_end = torch.cumsum(fcap, 0)
        slot_base = slot_end - fcap
        nb, slot_total, any_bc, any_cc = torch.stack([
            base[-1], slot_end[-1], (flags & N.FRAME_BLOCK_CHECKSUM).sum(),
            (flags & N.FRAME_CONTENT_CHECKSUM).sum()]).tolist()
        status = torch.where(S["status"] == N.FRAME_SKIPPABLE, torch.zeros_like(S["status"]), S["status"])
        if nb:
            R = N.frames_records(frames, off, ln, S, base, slot_base, n, nb)
            owner = R["frame"]
            in_chain = chain[owner]
            stored = (R["raw"] != 0) & ~in_chain
            slots = torch.empty(slot_total + 16, dtype=torch.uint8, device=dev)
            blk = torch.empty(nb, dtype=torch.int32, device=dev)
            # stored blocks and the chains' blocks go to the decoder with length 0 (rejected at once, no work)
            zlen = torch.zeros_like(R["len"])
            dec_len = torch.where(stored | in_chain, zlen, R["len"])
            count = torch.where(chain, S["nblocks"], torch.zeros_like(S["nblocks"]))
            if direct:
                # a block's size, as the frame's decoder would find it: at most the frame's block size
                # (lz4frame.c:1844-1847), else the block fails
                sized = torch.empty(nb, dtype=torch.int32, device=dev)
                N.launch_decompressed_size(frames, R["pos"], dec_len, sized, nb)
                fits = (sized >= 0) & (sized <= R["slot_cap"])
                N.launch_decompress_chains(frames, R["pos"], R["len"], R["raw"], base, count, slots, slot_base,
                                           maxb.to(torch.int32), blk, n)
                size = torch.where(stored, R["len"],
                                   torch.where(in_chain, blk.clamp(min=0), torch.where(fits, sized, zlen)))
            else:
                N.launch_decompress(frames, R["pos"], dec_len, slots, R["slot_off"], R["slot_cap"], blk, nb)
                N.launch_decompress_chains(frames, R["pos"], R["len"], R["raw"], base, count, slots, slot_base,
                                           maxb.to(torch.int32), blk, n)
                size = torch.where(stored, R["len"], blk.clamp(min=0))
            goff = N.exclusive_scan(size)
            out_off = goff[base[:-1]]
            out_len = goff[base[1:]] - out_off
            out_total = int(goff[-1])
            out = torch.empty(out_total + 16, dtype=torch.uint8, device=dev)
            zero = torch.zeros_like(size)
            if direct:
                here = torch.empty(nb, dtype=torch.int32, device=dev)
                N.launch_decompress(frames, R["pos"], torch.where(fits, dec_len, zlen), out, goff,
                                    torch.where(in_chain | stored, zero, size), here, nb)
                blk = torch.where(in_chain, blk, here)
                from_slot = slot_base[owner] + (goff[:nb] - out_off[owner])
                N.gather(slots, from_slot, torch.where(in_chain, size, zero), out, goff, nb)
            else:
                # a chain wrote its blocks back to back from its frame's first slot
                from_slot = torch.where(in_chain, slot_base[owner] + (goff[:nb] - out_off[owner]), R["slot_off"])
                N.gather(slots, from_slot, torch.where(stored, zero, size), out, goff, nb)
            bad = ((blk < 0) & ~stored).to(torch.int32)
            N.gather(frames, R["pos"], torch.where(stored, size, zero), out, goff, nb)
            fbad = torch.zeros(n, dtype=torch.int32, device=dev).index_add_(0, owner, bad)
            status = torch.where((status == 0) & (fbad > 0), torch.full_like(status, N.FRAME_BLOCK_FAILED), status)
            if any_bc:                                         # lz4frame.c:1819
                sums = torch.empty(nb, dtype=torch.int32, device=dev)
                N.launch_xxh32_batch(frames, R["pos"], R["len"].to(torch.int64), 0, sums, nb)
                crc_bad = (R["crc"] >= 0) & _crc_mismatch(frames, sums, R["crc"].clamp(min=0))
                fcrc = torch.zeros(n, dtype=torch.int32, device=dev).index_add_(0, owner, crc_bad.to(torch.int32))
                status = torch.where((status == 0) & (fcrc > 0),
                                     torch.full_like(status, N.FRAME_BLOCK_CHECKSUM_BAD), status)
        else:
            out = torch.empty(16, dtype=torch.uint8, device=dev)
            out_total = 0
            out_off = torch.zeros(n, dtype=torch.int64, device=dev)
            out_len = torch.zeros(n, dtype=torch.int64, device=dev)
        wrong = (S["content_size"] != 0) & (S["content_size"] != out_len)      # lz4frame.c:1927
        status = torch.where((status == 0) & wrong, torch.full_like(status, N.FRAME_CONTENT_SIZE_WRONG), status)
        if any_cc:                                             # lz4frame.c:1850, 1959-1964
            sums = torch.empty(n, dtype=torch.int32, device=dev)
            N.launch_xxh32_batch(out, out_off, out_len, 0, sums, n)
            cc_bad = (S["cpos"] >= 0) & _crc_mismatch(frames, sums, S["cpos"].clamp(min=0))
            status = torch.where((status == 0) & cc_bad, torch.full_like(status, N.FRAME_CONTENT_CHECKSUM_BAD),
                                 status)
        return out[:out_total], out_off, out_len, status, S["end"]


def _stage_many(views):
    """The buffers packed back to back on the device through the block API's
    pinned staging (one host-to-device copy): (device bytes, int64 offsets,
    int32 lengths)."""
    from ..block import _block as B
    lens = [v.nbytes for v in views]
    zeros = [0] * len(views)
    lay, _h, d = B._stage_in(N.device(), views, B._excl_offsets(lens), lens, zeros, zeros)
    buf, d_off, d_len = B._dev_views(lay, d, len(views))[:3]
    return buf[:sum(lens)] if sum(lens) else buf[:0], d_off, d_len


def compress_many(datas, compression_level=0, block_size=0, content_checksum=False, block_checksum=False,
                  block_linked=True, store_size=True, return_bytearray=False):
    """[compress(d, ...) for d in datas] in one batched call (compress_batch
    on the inputs packed into one staging copy).  Levels >= 3 raise what
    ``compress`` raises."""
    views = [_buffer(d, "data") for d in datas]
    level = _c_int(compression_level, "compression_level")
    bsid_req = _c_int(block_size, "block_size")
    if not views:
        return []
    if max(v.nbytes for v in views) > 0x7FFFFFFF:   # a frame beyond the staging tables: the single-frame path
        return [compress(v, level, bsid_req, content_checksum, block_checksum, block_linked, store_size,
                         return_bytearray) for v in views]
    N.device()
    resolve_parse("exact", level, block_linked)
    buf, d_off, d_len = _stage_many(views)
    frames, f_off, f_len = compress_batch(buf, d_off, d_len, compression_level=level, block_size=bsid_req,
                                          content_checksum=content_checksum, block_checksum=block_checksum,
                                          block_linked=block_linked, store_size=store_size)
    return _unpack_many(frames, f_off, f_len, bool(return_bytearray))


def _unpack_many(buf, off, length, as_bytearray):
    """New bytes objects of the spans of a device buffer (one device-to-host copy, one pooled host copy)."""
    from ..block import _block as B
    host = buf.cpu().numpy()
    return B._results_many(host, off.cpu().tolist(), length.cpu().tolist(), None, as_bytearray)


def decompress_many(frames, return_bytearray=False, return_bytes_read=False, direct: bool = False):
    """[decompress(f, ...) for f in frames] in one batched call
    (decompress_batch; ``direct`` as there).  If a frame fails, the lowest
    failing index raises what ``decompress`` raises for its bytes."""
    views = [_buffer(f, "data") for f in frames]
    if not views:
        return []
    if max(v.nbytes for v in views) > 0x7FFFFFFF:
        return [decompress(v, return_bytearray, return_bytes_read) for v in views]
    buf, d_off, d_len = _stage_many(views)
    out, o_off, o_len, status, read = decompress_batch(buf, d_off, d_len, direct=direct)
    st = status.cpu().tolist()
    for i, s in enumerate(st):
        if s != 0:
            decompress(views[i])                               # raises the single call's error
            raise RuntimeError(f"lz4.frame.decompress_many: frame {i} failed with batch status {s}, "
                               "but decompress accepts it")
    res = _unpack_many(out, o_off, o_len, bool(return_bytearray))
    if return_bytes_read:
        return list(zip(res, read.cpu().tolist()))
    return res

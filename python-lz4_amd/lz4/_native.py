"""Binding to the HIP C-ABI library ``_lz4m.so`` (include/lz4m.h).

The library is loaded into the process's HIP runtime -- the one PyTorch-ROCm
already loaded (same SONAME, libamdhip64.so.7) -- so device pointers of torch
tensors and torch's current HIP stream are passed straight through.

There is no CPU code path behind this module: if the library or a HIP device
is missing, every entry point raises ``RuntimeError``.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import threading

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lz4m.so")

TABLE_U16_HASH4 = 0
TABLE_U32_HASH5 = 1
TABLE_AUTO = 2
PARSE_PARALLEL = 3   # parallel-parse compressor: valid blocks, ratio of LZ4_compress_default
PARSE_PARALLEL_LARGE = 4   # the same for blocks > 64 KiB
PARSE_PARALLEL_HQ = 5   # PARSE_PARALLEL with the reference's 13-bit table (ratio of LZ4_compress_default)
LINKED_SERIAL = 1        # lz4m_compress_linked_batch modes
LINKED_SPECULATIVE = 2
EINVAL = 0x10000
# decoder selector of lz4m_decompress_batch_sel (include/lz4m.h)
DECODERS = {"auto": 0, "hist": 3, "rows": 4}
# walk selector of lz4m_decompressed_size_batch, and its status for a size above INT32_MAX
WALKS = {"auto": 0, "lane": 1, "wave": 2}
SIZE_OVERFLOW = -(2**31)

_lock = threading.Lock()
_lib = None


def _declare(lib) -> None:
    vp, i32, i64, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32
    sig = {
        "lz4m_compress_bound": ([i32], i32),
        "lz4m_selftest_lds_order": ([], i32),
        "lz4m_version_number": ([], i32),
        "lz4m_version_string": ([], C.c_char_p),
        "lz4m_decompress_batch": ([vp, vp, vp, vp, vp, vp, vp, i64, vp], i32),
        "lz4m_decompress_workspace_bytes": ([], C.c_size_t),
        "lz4m_decompress_batch_ws": ([vp, vp, vp, vp, vp, vp, vp, i64, vp, C.c_size_t, vp], i32),
        "lz4m_decompress_workspace_size": ([i64, i64], C.c_size_t),
        "lz4m_decompress_batch_sel": ([vp, vp, vp, vp, vp, vp, vp, i64, vp, C.c_size_t, i32, vp], i32),
        "lz4m_decompress_batch_dict": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp], i32),
        "lz4m_decompress_batch_prefix": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp], i32),
        "lz4m_decompressed_size_batch": ([vp, vp, vp, vp, vp, i64, i32, vp], i32),
        "lz4m_decompress_chain": ([vp, vp, vp, vp, vp, vp, i64, i32, vp], i32),
        "lz4m_compress_batch": ([vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, vp], i32),
        "lz4m_compress_dict_batch": ([vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp], i32),
        "lz4m_compress_prefix_batch": ([vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp], i32),
        "lz4m_compress_linked_workspace_size": ([i64], C.c_size_t),
        "lz4m_compress_linked_passes": ([], i32),
        "lz4m_pcompress_large_workspace_size": ([i64, i32], C.c_size_t),
        "lz4m_pcompress_large_batch": ([vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, C.c_size_t, vp], i32),
        "lz4m_pcompress_dict_table_bytes": ([], C.c_size_t),
        "lz4m_pcompress_dict_prepare": ([vp, i64, vp, C.c_size_t, vp], i32),
        "lz4m_pcompress_dict_batch": ([vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp], i32),
        "lz4m_compress_linked_batch": ([vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, vp, C.c_size_t, vp], i32),
        "lz4m_compress_hc_workspace_size": ([i64, i32], C.c_size_t),
        "lz4m_compress_hc_batch": ([vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, C.c_size_t, vp], i32),
        "lz4m_compress_opt_workspace_size": ([i64, i32], C.c_size_t),
        "lz4m_compress_opt_batch": ([vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, C.c_size_t, vp], i32),
        "lz4m_compress_hc_dict_workspace_size": ([i64, i32], C.c_size_t),
        "lz4m_compress_hc_dict_batch": ([vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp, C.c_size_t, vp], i32),
        "lz4m_xxh32_batch": ([vp, vp, vp, u32, vp, i64, vp], i32),
        "lz4m_xxh32_long": ([vp, i64, u32, vp, vp], i32),
        "lz4m_scan_scratch_entries": ([i64], i64),
        "lz4m_exclusive_scan": ([vp, i64, i64, vp, vp, i64, vp], i32),
        "lz4m_gather": ([vp, vp, vp, vp, vp, i64, vp], i32),
        "lz4m_frame_block_sizes": ([vp, vp, i32, vp, i64, vp], i32),
        "lz4m_frame_emit": ([vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, vp], i32),
        "lz4m_frame_scan": ([vp, i64, i64, i32, i32, i32, i64, vp, vp, vp, vp, vp, vp], i32),
        "lz4m_frames_scan": ([vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp], i32),
        "lz4m_frames_records": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp], i32),
        "lz4m_decompress_chains": ([vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp], i32),
        "lz4m_frames_plan": ([vp, i64, i32, i32, vp, vp, vp, vp], i32),
        "lz4m_frames_plan_blocks": ([vp, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp], i32),
        "lz4m_frames_sizes": ([vp, vp, vp, i32, i32, i64, vp, vp, vp], i32),
        "lz4m_frames_emit": ([vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, i64, vp], i32),
        "lz4m_decompress_safe": ([vp, vp, i32, i32], i32),
        "lz4m_compress_default": ([vp, vp, i32, i32], i32),
        "lz4m_compress_block_api": ([vp, vp, i32, i32, i32], i32),
        "lz4m_decompress_safe_staged": ([vp, i32, i32, C.POINTER(vp)], i32),
        "lz4m_compress_block_api_staged": ([vp, i32, i32, i32, i32, C.POINTER(vp)], i32),
        "lz4m_xxh32": ([vp, C.c_size_t, u32], u32),
        "lz4m_xxh32_host_reset": ([vp, u32], None),
        "lz4m_xxh32_host_update": ([vp, vp, C.c_size_t], None),
        "lz4m_xxh32_host_digest": ([vp], u32),
        "lz4m_xxh32_host": ([vp, C.c_size_t, u32], u32),
        "lz4m_host_copy": ([vp, vp, C.c_size_t, i32, vp], None),
        "lz4m_host_copy_many": ([vp, vp, vp, C.c_size_t, i32], None),
        "lz4m_single_call_worker": ([i32], i32),
        "lz4m_single_call_worker_state": ([vp], i32),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res


def lib():
    """The loaded C-ABI library (raises if it is missing)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"lz4 MI355X backend not built: {LIB_PATH} is missing "
                        "(run `make -C python-lz4_amd/csrc` or __graft_entry__.build())")
                l = C.CDLL(LIB_PATH)
                _declare(l)
                _lib = l
    return _lib


def device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("lz4 MI355X backend: no HIP device is visible; this package has no CPU code path")
    return torch.device("cuda", torch.cuda.current_device())


_GPU_SEEN = False


def require_device() -> None:
    """device()'s check for the single-call entry points, which pick the
    current HIP device in C: after the first success it costs nothing
    (torch.cuda.is_available + current_device are ~3 us of a ~50 us call)."""
    global _GPU_SEEN
    if not _GPU_SEEN:
        device()
        _GPU_SEEN = True


def stream_ptr(stream=None) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else int(t.data_ptr())


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed to launch (code {rc:#x})")


def compress_bound(n: int) -> int:
    """LZ4_compressBound (lz4.h:212)."""
    return 0 if n < 0 or n > 0x7E000000 else n + n // 255 + 16


# ------------------------------------------------------------ raw launchers
def launch_decompress(src, src_off, src_len, dst, dst_off, dst_cap, status, n, stream=None,
                      dict_buf=None, dict_off=None, dict_len=None, decoder: str = "auto",
                      src_bytes: int | None = None) -> None:
    """Batched LZ4_decompress_safe(_usingDict).  ``decoder`` forces one of the
    decoders (``DECODERS``; "auto" picks by batch size); ``src_bytes`` bounds
    the blocks' total compressed size (default: all of ``src``) and sizes the
    large-batch decoder's scratch."""
    L = lib()
    sp = stream_ptr(stream)
    if dict_buf is None:
        work = _workspace(src.device, stream, n, src.numel() if src_bytes is None else src_bytes)
        rc = L.lz4m_decompress_batch_sel(ptr(src), ptr(src_off), ptr(src_len), ptr(dst), ptr(dst_off), ptr(dst_cap),
                                         ptr(status), n, ptr(work), work.numel(), DECODERS[decoder], sp)
    else:
        rc = L.lz4m_decompress_batch_dict(ptr(src), ptr(src_off), ptr(src_len), ptr(dst), ptr(dst_off),
                                          ptr(dst_cap), ptr(dict_buf), ptr(dict_off), ptr(dict_len), ptr(status),
                                          n, sp)
    check(rc, "lz4m_decompress_batch")


def launch_decompressed_size(src, src_off, src_len, size, n, stream=None, dict_len=None, walk: str = "auto") -> None:
    """Decoded sizes without decoding (lz4m_decompressed_size_batch): size[i]
    = what the decoders report for block i at a capacity large enough not to
    matter, with ``dict_len`` (int32[n] or None) bytes of dictionary.
    ``walk``: a key of ``WALKS``."""
    if walk not in WALKS:
        raise ValueError(f"walk must be one of {sorted(WALKS)}, not {walk!r}")
    check(lib().lz4m_decompressed_size_batch(ptr(src), ptr(src_off), ptr(src_len), ptr(dict_len), ptr(size), n,
                                             WALKS[walk], stream_ptr(stream)),
          "lz4m_decompressed_size_batch")


_WORK: "collections.OrderedDict" = collections.OrderedDict()
_WORK_STREAMS = 4   # scratch buffers kept (least recently used streams dropped first)


def _workspace(dev, stream, n: int = 0, src_bytes: int = 0) -> torch.Tensor:
    """Decoder scratch (lz4m_decompress_workspace_size), one buffer per
    (device, stream), grown on demand: calls on one stream are ordered, so
    they can share it.  The buffer is allocated on the stream that uses it,
    so when it is dropped (regrowth, eviction, release_workspaces) the
    caching allocator hands its memory only to work ordered after that
    stream's pending launches.  At most _WORK_STREAMS buffers are cached."""
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    key = (dev, int(s.cuda_stream))
    need = int(lib().lz4m_decompress_workspace_size(n, src_bytes))
    w = _WORK.pop(key, None)
    if w is None or w.numel() < need:
        w = None
        w = _empty_on(s, need, dev)
    _WORK[key] = w
    while len(_WORK) > _WORK_STREAMS:
        _WORK.popitem(last=False)
    return w


def _empty_on(stream, nbytes: int, dev) -> torch.Tensor:
    """uint8 scratch allocated on the stream that uses it (None: the current
    one): when it is dropped the caching allocator hands its memory only to
    work ordered after that stream's pending launches."""
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
        return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


def release_workspaces() -> None:
    """Drop the cached decoder scratch (it grows to ~1/3 of the largest
    compressed batch decoded)."""
    _WORK.clear()


def launch_decompress_prefix(src, src_off, src_len, dst, dst_off, dst_cap, dict_base, dict_len, status, n,
                             stream=None) -> None:
    """Batched LZ4_decompress_safe_usingDict, block i's dictionary the
    dict_len[i] bytes ending at offset dst_off[i] of ``dict_base`` (laid out
    like ``dst``; lz4m_decompress_batch_prefix)."""
    check(lib().lz4m_decompress_batch_prefix(ptr(src), ptr(src_off), ptr(src_len), ptr(dst), ptr(dst_off),
                                             ptr(dst_cap), ptr(dict_base), ptr(dict_len), ptr(status), n,
                                             stream_ptr(stream)),
          "lz4m_decompress_batch_prefix")


def launch_decompress_chain(src, src_off, src_len, raw_mask, dst, status, n, max_block, stream=None) -> None:
    raw = raw_mask.to(torch.uint8)
    rc = lib().lz4m_decompress_chain(ptr(src), ptr(src_off), ptr(src_len), ptr(raw), ptr(dst), ptr(status), n,
                                     max_block, stream_ptr(stream))
    check(rc, "lz4m_decompress_chain")


def launch_compress(src, src_off, src_len, dst, dst_off, dst_cap, out_len, n, table, accel, stream=None,
                    max_len: int | None = None) -> None:
    """Batched compression (lz4m_compress_batch).  PARSE_PARALLEL_LARGE with
    ``max_len`` (the longest block) parses each block as up to 16 segments
    (lz4m_pcompress_large_batch)."""
    L = lib()
    if table == PARSE_PARALLEL_LARGE and max_len is not None:
        work = _empty_on(stream, L.lz4m_pcompress_large_workspace_size(n, max_len), src.device)
        rc = L.lz4m_pcompress_large_batch(ptr(src), ptr(src_off), ptr(src_len), ptr(dst), ptr(dst_off),
                                          ptr(dst_cap), ptr(out_len), n, max_len, ptr(work), work.numel(),
                                          stream_ptr(stream))
        check(rc, "lz4m_pcompress_large_batch")
        return
    rc = L.lz4m_compress_batch(ptr(src), ptr(src_off), ptr(src_len), ptr(dst), ptr(dst_off), ptr(dst_cap),
                               ptr(out_len), n, table, accel, stream_ptr(stream))
    check(rc, "lz4m_compress_batch")


def launch_compress_dict(src, src_off, src_len, dict_len, dst, dst_off, dst_cap, out_len, n, accel,
                         stream=None, prefix: bool = False) -> None:
    """lz4.block.compress(dict=) per block; the dictionary tail precedes each block in ``src``.
    ``prefix``: the caller's dictionary ends where the source begins (prefix mode,
    lz4m_compress_prefix_batch)."""
    name = "lz4m_compress_prefix_batch" if prefix else "lz4m_compress_dict_batch"
    rc = getattr(lib(), name)(ptr(src), ptr(src_off), ptr(src_len), ptr(dict_len), ptr(dst), ptr(dst_off),
                              ptr(dst_cap), ptr(out_len), n, accel, stream_ptr(stream))
    check(rc, name)


def pcompress_dict_prepare(dict_buf: torch.Tensor, stream=None) -> torch.Tensor:
    """The 8 KiB table of a device-resident dictionary (its last 64 KiB count)
    for launch_pcompress_dict (lz4m_pcompress_dict_prepare), stream-ordered."""
    L = lib()
    table = _empty_on(stream, L.lz4m_pcompress_dict_table_bytes(), dict_buf.device)
    n = dict_buf.numel()
    check(L.lz4m_pcompress_dict_prepare(ptr(dict_buf) if n else None, n, ptr(table), table.numel(), stream_ptr(stream)),
          "lz4m_pcompress_dict_prepare")
    return table


def launch_pcompress_dict(src, src_off, src_len, dict_buf, table, dst, dst_off, dst_cap, out_len, n,
                          stream=None) -> None:
    """PARSE_PARALLEL with ``dict_buf`` (uint8, device) as the one dictionary
    of all n blocks and ``table`` = pcompress_dict_prepare(dict_buf)
    (lz4m_pcompress_dict_batch); the blocks decode with that dictionary."""
    nd = dict_buf.numel()
    rc = lib().lz4m_pcompress_dict_batch(ptr(src), ptr(src_off), ptr(src_len), ptr(dict_buf) if nd else None, nd,
                                         ptr(table), ptr(dst), ptr(dst_off), ptr(dst_cap), ptr(out_len), n,
                                         stream_ptr(stream))
    check(rc, "lz4m_pcompress_dict_batch")


def launch_compress_hc(src, src_off, src_len, dst, dst_off, dst_cap, out_len, n, level: int = 9, stream=None,
                       max_len: int = 0, dict_len=None) -> None:
    """Batched hash-chain (HC) compression (lz4m_compress_hc_batch): valid
    blocks near the size of LZ4_compress_HC at ``level``, not byte-identical
    to it.  With ``dict_len`` (int32[n], lz4m_compress_hc_dict_batch) block i
    has history: the last min(dict_len[i], 65536) bytes of its dictionary
    precede it in ``src`` (as for launch_compress_dict); dict_len[i] <= 0: no
    history.  The chain workspace (256 KiB per block; 320 MiB at most, 640
    with history) is allocated per call on the stream that uses it, from
    torch's caching allocator."""
    name = "lz4m_compress_hc_batch" if dict_len is None else "lz4m_compress_hc_dict_batch"
    size = "lz4m_compress_hc_workspace_size" if dict_len is None else "lz4m_compress_hc_dict_workspace_size"
    p = ptr if n > 0 else (lambda t: None)   # an empty batch passes no pointers
    work = _empty_on(stream, getattr(lib(), size)(n, max_len), src.device) if n > 0 else None
    hist = () if dict_len is None else (p(dict_len),)
    rc = getattr(lib(), name)(p(src), p(src_off), p(src_len), *hist, p(dst), p(dst_off), p(dst_cap), p(out_len), n,
                              level, ptr(work), 0 if work is None else work.numel(), stream_ptr(stream))
    check(rc, name)


def launch_compress_opt(src, src_off, src_len, dst, dst_off, dst_cap, out_len, n, level: int = 9, stream=None,
                        max_len: int | None = None) -> None:
    """Batched optimal-parse compression (lz4m_compress_opt_batch): valid
    blocks within 1 % of LZ4_compress_HC(12) at level 9, not byte-identical to
    it.  ``max_len`` is the longest block; None reads it back from ``src_len``
    (one host synchronisation).  The workspace (10 bytes per position for each
    of min(n, 2560) wavefronts: 1.6 GiB at most for 64 KiB blocks) is
    allocated per call on the stream that uses it, from torch's caching
    allocator."""
    if n <= 0:
        check(lib().lz4m_compress_opt_batch(None, None, None, None, None, None, None, n, level, None, 0,
                                            stream_ptr(stream)), "lz4m_compress_opt_batch")
        return
    if max_len is None:
        max_len = max(int(src_len.max().item()), 0)
    work = _empty_on(stream, lib().lz4m_compress_opt_workspace_size(n, max_len), src.device)
    rc = lib().lz4m_compress_opt_batch(ptr(src), ptr(src_off), ptr(src_len), ptr(dst), ptr(dst_off), ptr(dst_cap),
                                       ptr(out_len), n, level, ptr(work), work.numel(), stream_ptr(stream))
    check(rc, "lz4m_compress_opt_batch")


def launch_compress_linked(src, src_off, src_len, link, dst, dst_off, dst_cap, out_len, n, accel,
                           mode: int = LINKED_SPECULATIVE, stream=None) -> None:
    """Linked-block streams (lz4m_compress_linked_batch).  The speculative
    mode synchronises ``stream`` once per pass."""
    L = lib()
    work = None
    if mode == LINKED_SPECULATIVE:
        work = _empty_on(stream, L.lz4m_compress_linked_workspace_size(n), src.device)
    rc = L.lz4m_compress_linked_batch(ptr(src), ptr(src_off), ptr(src_len), ptr(link), ptr(dst), ptr(dst_off),
                                      ptr(dst_cap), ptr(out_len), n, accel, mode, ptr(work),
                                      0 if work is None else work.numel(), stream_ptr(stream))
    check(rc, "lz4m_compress_linked_batch")


class Parse(collections.namedtuple("Parse", "launcher table accel level history prefix",
                                    defaults=(TABLE_AUTO, 1, 0, "", False))):
    """What lz4.block's and lz4.frame's ``resolve_parse`` make of a compression
    call's arguments; ``launch_blocks`` dispatches on it.  launcher: "table"
    (the exact and parallel parses, by ``table`` and ``accel``), "hc" or "opt"
    (at ``level``).  history: which array goes with the blocks -- "" none;
    "hist" the length of each block's dictionary or history, whose last 64 KiB
    precede the block in the source (``prefix``: taken in prefix mode); "link"
    the link flags of linked frames' blocks; "shared" one PreparedDict."""
    __slots__ = ()


def _launch_hc(p, a, x, max_len, spec, s):
    launch_compress_hc(*a, p.level, s, max_len=max_len or 0, dict_len=x)


# (launcher, history) -> launch(parse, the eight batch arguments, extra, max_len, speculative, stream); a pair that
# is not here is a parse no resolver gives
_BLOCK_LAUNCH = {
    ("table", ""): lambda p, a, x, max_len, spec, s: launch_compress(*a, p.table, p.accel, s, max_len=max_len),
    ("table", "hist"): lambda p, a, x, max_len, spec, s: launch_compress_dict(*a[:3], x, *a[3:], p.accel, s,
                                                                              prefix=p.prefix),
    ("table", "link"): lambda p, a, x, max_len, spec, s: launch_compress_linked(
        *a[:3], x, *a[3:], p.accel, LINKED_SPECULATIVE if spec else LINKED_SERIAL, s),
    ("table", "shared"): lambda p, a, x, max_len, spec, s: launch_pcompress_dict(*a[:3], x.tail, x.table, *a[3:], s),
    ("hc", ""): _launch_hc, ("hc", "hist"): _launch_hc,
    ("opt", ""): lambda p, a, x, max_len, spec, s: launch_compress_opt(*a, p.level, s, max_len=max_len),
}


def launch_blocks(parse: Parse, src, src_off, src_len, dst, dst_off, dst_cap, out_len, n, *, extra=None,
                  max_len: int | None = None, speculative: bool = False, stream=None) -> None:
    """The one launch of block compression: n blocks with the parse ``parse``.
    ``extra`` is what ``parse.history`` names; ``max_len`` the longest block
    (sizes the workspaces of the large-block parallel, HC and optimal parses;
    None: unknown); ``speculative``: linked blocks compress speculatively in
    parallel, not one wavefront per frame."""
    _BLOCK_LAUNCH[parse.launcher, parse.history](parse, (src, src_off, src_len, dst, dst_off, dst_cap, out_len, n),
                                                 extra, max_len, speculative, stream)


def launch_xxh32_batch(src, off, length, seed, out, n, stream=None) -> None:
    rc = lib().lz4m_xxh32_batch(ptr(src), ptr(off), ptr(length), seed & 0xFFFFFFFF, ptr(out), n, stream_ptr(stream))
    check(rc, "lz4m_xxh32_batch")


def launch_xxh32_long(src, length, seed, out, stream=None) -> None:
    rc = lib().lz4m_xxh32_long(ptr(src), length, seed & 0xFFFFFFFF, ptr(out), stream_ptr(stream))
    check(rc, "lz4m_xxh32_long")


def exclusive_scan(lengths: torch.Tensor, add: int = 0, base: int = 0, stream=None) -> torch.Tensor:
    """int64 offsets (n+1 entries, last = total) of int32 ``lengths`` (+add each)."""
    n = lengths.numel()
    out = torch.empty(n + 1, dtype=torch.int64, device=lengths.device)
    scratch = torch.empty(int(lib().lz4m_scan_scratch_entries(n)), dtype=torch.int64, device=lengths.device)
    rc = lib().lz4m_exclusive_scan(ptr(lengths), add, base, ptr(out), ptr(scratch), n, stream_ptr(stream))
    check(rc, "lz4m_exclusive_scan")
    return out


def gather(src, src_off, length, out, out_off, n, stream=None) -> None:
    rc = lib().lz4m_gather(ptr(src), ptr(src_off), ptr(length), ptr(out), ptr(out_off), n, stream_ptr(stream))
    check(rc, "lz4m_gather")


def frame_block_sizes(raw_len, cmp_len, block_checksum, rec_len, n, stream=None) -> None:
    rc = lib().lz4m_frame_block_sizes(ptr(raw_len), ptr(cmp_len), int(bool(block_checksum)), ptr(rec_len), n,
                                      stream_ptr(stream))
    check(rc, "lz4m_frame_block_sizes")


def frame_emit(raw, raw_off, raw_len, cmp, cmp_off, cmp_len, frame, frame_off, block_checksum, n,
               stream=None) -> None:
    rc = lib().lz4m_frame_emit(ptr(raw), ptr(raw_off), ptr(raw_len), ptr(cmp), ptr(cmp_off), ptr(cmp_len),
                               ptr(frame), ptr(frame_off), int(bool(block_checksum)), n, stream_ptr(stream))
    check(rc, "lz4m_frame_emit")


def frame_scan(frame, frame_len, pos, block_checksum, content_checksum, max_block, max_rec, rec_pos, rec_len,
               rec_raw, rec_crc, result, stream=None) -> None:
    rc = lib().lz4m_frame_scan(ptr(frame), frame_len, pos, int(bool(block_checksum)), int(bool(content_checksum)),
                               max_block, max_rec, ptr(rec_pos), ptr(rec_len), ptr(rec_raw), ptr(rec_crc),
                               ptr(result), stream_ptr(stream))
    check(rc, "lz4m_frame_scan")


# status codes and flag bits of the batched frame calls (include/lz4m.h LZ4M_FRAME_*)
FRAME_OK, FRAME_SKIPPABLE = 0, 10
FRAME_BLOCK_FAILED, FRAME_BLOCK_CHECKSUM_BAD, FRAME_CONTENT_SIZE_WRONG, FRAME_CONTENT_CHECKSUM_BAD = 16, 17, 18, 19
FRAME_LINKED, FRAME_BLOCK_CHECKSUM, FRAME_CONTENT_CHECKSUM = 1, 2, 4


def frames_scan(buf, frame_off, frame_len, n, stream=None) -> dict:
    """lz4m_frames_scan over n frames: a dict of its per-frame output tensors."""
    dev = buf.device
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)   # noqa: E731
    i64 = lambda: torch.empty(n, dtype=torch.int64, device=dev)   # noqa: E731
    r = {"status": i32(), "nblocks": i32(), "hsize": i32(), "end": i64(), "cpos": i64(), "bsid": i32(),
         "flags": i32(), "content_size": i64()}
    rc = lib().lz4m_frames_scan(ptr(buf), ptr(frame_off), ptr(frame_len), n, ptr(r["status"]), ptr(r["nblocks"]),
                                ptr(r["hsize"]), ptr(r["end"]), ptr(r["cpos"]), ptr(r["bsid"]), ptr(r["flags"]),
                                ptr(r["content_size"]), stream_ptr(stream))
    check(rc, "lz4m_frames_scan")
    return r


def frames_records(buf, frame_off, frame_len, scan: dict, block_base, slot_base, n, n_blocks, stream=None) -> dict:
    """lz4m_frames_records: a dict of the per-block arrays (n_blocks entries each)."""
    dev = buf.device
    t = lambda dt: torch.empty(n_blocks, dtype=dt, device=dev)   # noqa: E731
    r = {"pos": t(torch.int64), "len": t(torch.int32), "raw": t(torch.uint8), "crc": t(torch.int64),
         "frame": t(torch.int64), "slot_off": t(torch.int64), "slot_cap": t(torch.int32)}
    rc = lib().lz4m_frames_records(ptr(buf), ptr(frame_off), ptr(frame_len), ptr(scan["nblocks"]),
                                   ptr(scan["hsize"]), ptr(scan["bsid"]), ptr(scan["flags"]), ptr(block_base),
                                   ptr(slot_base), n, ptr(r["pos"]), ptr(r["len"]), ptr(r["raw"]), ptr(r["crc"]),
                                   ptr(r["frame"]), ptr(r["slot_off"]), ptr(r["slot_cap"]), stream_ptr(stream))
    check(rc, "lz4m_frames_records")
    return r


def launch_decompress_chains(src, src_off, src_len, raw_flag, first, count, dst, dst_off, max_block, status,
                             n_chains, stream=None) -> None:
    rc = lib().lz4m_decompress_chains(ptr(src), ptr(src_off), ptr(src_len), ptr(raw_flag), ptr(first), ptr(count),
                                      ptr(dst), ptr(dst_off), ptr(max_block), ptr(status), n_chains,
                                      stream_ptr(stream))
    check(rc, "lz4m_decompress_chains")


def frames_plan(src_len, n, block_size_id: int, block_linked: bool, stream=None):
    """lz4m_frames_plan: (bsid, nblocks, linked), int32 per frame."""
    dev = src_len.device
    out = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3)]
    rc = lib().lz4m_frames_plan(ptr(src_len), n, block_size_id, int(bool(block_linked)), ptr(out[0]), ptr(out[1]),
                                ptr(out[2]), stream_ptr(stream))
    check(rc, "lz4m_frames_plan")
    return out


def frames_plan_blocks(src_off, src_len, bsid, linked, block_base, n, n_blocks, stream=None) -> dict:
    """lz4m_frames_plan_blocks: a dict of the per-block arrays."""
    dev = src_len.device
    t = lambda dt: torch.empty(n_blocks, dtype=dt, device=dev)   # noqa: E731
    r = {"raw_off": t(torch.int64), "raw_len": t(torch.int32), "cap": t(torch.int32), "link": t(torch.int32),
         "hist": t(torch.int32), "owner": t(torch.int64), "slot_len": t(torch.int32)}
    rc = lib().lz4m_frames_plan_blocks(ptr(src_off), ptr(src_len), ptr(bsid), ptr(linked), ptr(block_base), n,
                                       n_blocks, ptr(r["raw_off"]), ptr(r["raw_len"]), ptr(r["cap"]), ptr(r["link"]),
                                       ptr(r["hist"]), ptr(r["owner"]), ptr(r["slot_len"]), stream_ptr(stream))
    check(rc, "lz4m_frames_plan_blocks")
    return r


def frames_sizes(rec_off, block_base, src_len, store_size, content_checksum, n, stream=None):
    """lz4m_frames_sizes: (hsize int32, frame_size int64) per frame."""
    hsize = torch.empty(n, dtype=torch.int32, device=src_len.device)
    size = torch.empty(n, dtype=torch.int64, device=src_len.device)
    rc = lib().lz4m_frames_sizes(ptr(rec_off), ptr(block_base), ptr(src_len), int(bool(store_size)),
                                 int(bool(content_checksum)), n, ptr(hsize), ptr(size), stream_ptr(stream))
    check(rc, "lz4m_frames_sizes")
    return hsize, size


def frames_emit(frames, frame_off, frame_size, bsid, linked, src_len, store_size, block_checksum, content_checksum,
                content_hash, n, stream=None) -> None:
    rc = lib().lz4m_frames_emit(ptr(frames), ptr(frame_off), ptr(frame_size), ptr(bsid), ptr(linked), ptr(src_len),
                                int(bool(store_size)), int(bool(block_checksum)), int(bool(content_checksum)),
                                ptr(content_hash), n, stream_ptr(stream))
    check(rc, "lz4m_frames_emit")


# ------------------------------------------------------------ host XXH32
_probe = b"lz4m"
_BYTES_DATA = C.cast(C.c_char_p(_probe), C.c_void_p).value - id(_probe)   # measured, not assumed
del _probe


def host_addr(view: memoryview):
    """Address of a contiguous host buffer (read-only ones too), None if empty;
    it holds while the caller keeps ``view``.  A whole bytes object (its data
    offset measured at import) or a writable buffer takes a fast path; numpy's
    .ctypes (~2.6 us) serves the rest."""
    if not view.nbytes:
        return None
    obj = view.obj
    if type(obj) is bytes and view.nbytes == len(obj):
        return id(obj) + _BYTES_DATA   # CPython: the bytes' data sits at a fixed offset in the object
    if not view.readonly:
        return C.addressof(C.c_char.from_buffer(view))
    return int(np.frombuffer(view, dtype=np.uint8).ctypes.data)


class HostXXH32:
    """Streaming XXH32 on a host core (include/lz4m.h lz4m_xxh32_host_*).
    ctypes drops the GIL during each update, so it runs beside GPU work
    issued from other threads."""

    def __init__(self, seed: int = 0):
        self._st = (C.c_uint32 * 12)()
        lib().lz4m_xxh32_host_reset(self._st, seed & 0xFFFFFFFF)

    def update(self, buf, n: int | None = None) -> None:
        mv = memoryview(buf).cast("B")
        lib().lz4m_xxh32_host_update(self._st, host_addr(mv), mv.nbytes if n is None else n)

    def update_ptr(self, ptr: int, n: int) -> None:
        lib().lz4m_xxh32_host_update(self._st, ptr, n)

    def digest(self) -> int:
        return int(lib().lz4m_xxh32_host_digest(self._st))


def xxh32_host(buf, seed: int = 0) -> int:
    """One-shot XXH32 of a host buffer on the calling host core."""
    mv = memoryview(buf).cast("B")
    return int(lib().lz4m_xxh32_host(host_addr(mv), mv.nbytes, seed & 0xFFFFFFFF))


_PIN = {}
_PIN_LOCK = threading.Lock()


def _pinned_pair(chunk: int):
    """Two pinned host buffers of `chunk` bytes from a process-wide pool
    (pinning 128 MiB costs tens of ms: never per call or per thread)."""
    with _PIN_LOCK:
        free = _PIN.setdefault(chunk, [])
        if free:
            return free.pop()
    return [torch.empty(chunk, dtype=torch.uint8, pin_memory=True) for _ in range(2)]


def _pinned_release(chunk: int, bufs) -> None:
    with _PIN_LOCK:
        _PIN.setdefault(chunk, []).append(bufs)


# The hashing copies run on a high-priority stream: HIP multiplexes
# same-priority streams over a few hardware queues (GPU_MAX_HW_QUEUES), and
# a copy stream on the compressing stream's queue ran its copies after the
# kernel -- the config-4 frame with a content checksum measured 8.4 GiB/s in
# the full bench, 11.9 with this
_HASH_STREAM_PRIORITY = -1

def xxh32_of_device(t: torch.Tensor, n: int, seed: int = 0, wait_stream=None, chunk: int = 64 << 20,
                    wait_event=None) -> int:
    """XXH32 of the first n bytes of a device tensor, hashed on a host core
    (xxh32_of_device_spans over the one span [0, n)).
    ``wait_event``: an event recorded when t was ready (preferred: a caller
    running this in a thread records it before queueing more work), else
    ``wait_stream``: the stream that produced t (default: current)."""
    if n <= 0:
        return HostXXH32(seed).digest()
    if wait_event is None:
        wait_event = torch.cuda.Event()
        wait_event.record(wait_stream if wait_stream is not None else torch.cuda.current_stream(t.device))
    return xxh32_of_device_spans(t, [(0, n, wait_event)], seed, chunk=chunk).digest()


def xxh32_of_device_spans(t: torch.Tensor, spans, seed: int = 0, state: "HostXXH32 | None" = None,
                          chunk: int = 64 << 20) -> "HostXXH32":
    """Continue an XXH32 on a host core over device bytes t[lo:hi] of each
    span (lo, hi, event) in order, the spans contiguous: a span's copies are
    queued behind its event (the device work that writes those bytes), so
    the hash follows the producer instead of waiting for all of it.  Chunks
    are copied to two pinned buffers on a side stream, each hashed while the
    next one copies (PCIe ~50 GB/s against ~13 GB/s of hashing).  Returns
    the state (``.digest()`` ends it)."""
    st = state if state is not None else HostXXH32(seed)
    pieces = []
    for lo, hi, ev in spans:
        for a in range(lo, hi, chunk):
            pieces.append((a, min(hi, a + chunk), ev))
    if pieces:
        side = torch.cuda.Stream(t.device, priority=_HASH_STREAM_PRIORITY)
        _drain_chunks(t.view(-1), pieces, side, chunk, lambda p, lo, hi: st.update_ptr(p, hi - lo))
    return st


def _drain_chunks(flat: torch.Tensor, pieces, side, chunk: int, consume) -> None:
    """Device bytes flat[lo:hi] of each piece (lo, hi, event or None), at most
    ``chunk`` bytes each, to the host in order: copied to two pinned buffers
    on the stream ``side``, piece i + 1 in flight while ``consume(pinned
    address, lo, hi)`` takes piece i.  A piece's copy is queued behind its
    event, each distinct event waited for once.  On an error too, the pinned
    pair goes back to the pool only once no copy can still write it."""
    bufs = _pinned_pair(chunk)
    evs = [torch.cuda.Event(), torch.cuda.Event()]
    waited = set()

    def issue(i):
        lo, hi, ev = pieces[i]
        with torch.cuda.stream(side):
            if ev is not None and id(ev) not in waited:
                side.wait_event(ev)
                waited.add(id(ev))
            bufs[i & 1][: hi - lo].copy_(flat[lo:hi], non_blocking=True)
            evs[i & 1].record(side)

    try:
        issue(0)
        for i, (lo, hi, _ev) in enumerate(pieces):
            if i + 1 < len(pieces):
                issue(i + 1)   # its buffer was consumed in iteration i - 1
            evs[i & 1].synchronize()
            consume(bufs[i & 1].data_ptr(), lo, hi)
    finally:
        for e in evs:
            e.synchronize()
        _pinned_release(chunk, bufs)


# ------------------------------------------------------------ host <-> device
# Large host <-> device moves (the drop-in frame calls on Python bytes) go
# through two pinned chunks: lz4m_host_copy fills / drains a chunk with a few
# host threads while the other chunk's DMA runs on a side stream; a content
# checksum can ride along (hashed from the chunk while it is copied).
_BIG = 32 << 20
_CHUNK = 64 << 20


def _copy_threads() -> int:
    try:
        vis = len(os.sched_getaffinity(0))
    except AttributeError:
        vis = os.cpu_count() or 1
    share = int(os.environ.get("OMP_NUM_THREADS", "16") or 16)
    return max(1, min(8, vis, share) - 1)   # one core left for the hash thread


def to_device(buf, dev=None, pad: int = 0) -> torch.Tensor:
    """Copy a bytes-like object to a device uint8 tensor (+pad zero bytes)."""
    dev = dev or device()
    mv = memoryview(buf).cast("B")
    n = mv.nbytes
    out = torch.empty(n + pad, dtype=torch.uint8, device=dev)
    if n >= _BIG:
        src = host_addr(mv)
        bufs = _pinned_pair(_CHUNK)
        evs = [None, None]
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        thr = _copy_threads()
        try:
            for i, lo in enumerate(range(0, n, _CHUNK)):
                hi = min(n, lo + _CHUNK)
                b = bufs[i & 1]
                if evs[i & 1] is not None:
                    evs[i & 1].synchronize()   # this chunk's previous DMA has read it
                lib().lz4m_host_copy(b.data_ptr(), src + lo, hi - lo, thr, None)
                with torch.cuda.stream(side):
                    out[lo:hi].copy_(b[: hi - lo], non_blocking=True)
                    evs[i & 1] = torch.cuda.Event()
                    evs[i & 1].record(side)
            torch.cuda.current_stream(dev).wait_stream(side)
        finally:
            for e in evs:
                if e is not None:
                    e.synchronize()
            _pinned_release(_CHUNK, bufs)
    elif n:
        import warnings
        with warnings.catch_warnings():   # read-only bytes: shared, only read
            warnings.simplefilter("ignore")
            host = torch.frombuffer(mv, dtype=torch.uint8)
        out[:n].copy_(host, non_blocking=False)
    if pad:
        out[n:].zero_()
    return out


_PyBytes_New = C.pythonapi.PyBytes_FromStringAndSize
_PyBytes_New.restype = C.py_object
_PyBytes_New.argtypes = [C.c_void_p, C.c_ssize_t]
_PyByteArray_New = C.pythonapi.PyByteArray_FromStringAndSize
_PyByteArray_New.restype = C.py_object
_PyByteArray_New.argtypes = [C.c_void_p, C.c_ssize_t]


_MADV_HUGEPAGE = 14
_HUGE = 2 << 20
_libc = None


def _advise_huge(addr: int, n: int) -> None:
    """Ask for transparent huge pages on the 2 MiB-aligned interior of a
    fresh host buffer (best effort).  Its first touch is the copy that fills
    it: with 4 KiB pages 8 GiB filled at 18 GB/s (a fault and a page zeroing
    per 4 KiB), with huge pages at 97 GB/s on the same 7 copy threads
    (profiles/r05/r05ab/fault.log; the GPU box runs THP in madvise mode)."""
    global _libc
    a = (addr + _HUGE - 1) & ~(_HUGE - 1)
    ln = (addr + n - a) & ~(_HUGE - 1)
    if ln <= 0 or os.environ.get("LZ4M_HUGEPAGES", "1") == "0":
        return
    if _libc is None:
        _libc = C.CDLL(None, use_errno=True)
        _libc.madvise.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
        _libc.madvise.restype = C.c_int
    _libc.madvise(a, ln, _MADV_HUGEPAGE)


def _new_host_buffer(n: int, as_bytearray: bool):
    """An uninitialised bytes (or bytearray) of n bytes and its data address
    (filled before anyone else sees it; huge pages asked for when large)."""
    if as_bytearray:
        ba = _PyByteArray_New(None, n)
        addr = C.addressof((C.c_char * n).from_buffer(ba))
        obj = ba
    else:
        obj = _PyBytes_New(None, n)
        addr = id(obj) + _BYTES_DATA
    if n >= 4 * _HUGE:
        _advise_huge(addr, n)
    return obj, addr


def to_host_bytes(t: torch.Tensor, n: int, as_bytearray: bool = False, hash_seed: int | None = None):
    """The first n bytes of a device tensor as a new bytes (or bytearray).
    hash_seed: also return the XXH32 of those bytes, hashed on a host core
    from each staged chunk while it is copied -> (bytes, digest)."""
    if n <= 0:
        out = bytearray() if as_bytearray else b""
        return (out, HostXXH32(hash_seed).digest()) if hash_seed is not None else out
    if n < _BIG:
        h = t.view(-1)[:n].cpu().numpy()
        out = bytearray(h.tobytes()) if as_bytearray else h.tobytes()
        return (out, xxh32_host(out, hash_seed)) if hash_seed is not None else out
    out, dst = _new_host_buffer(n, as_bytearray)
    st = HostXXH32(hash_seed) if hash_seed is not None else None
    side = torch.cuda.Stream(t.device)
    side.wait_stream(torch.cuda.current_stream(t.device))
    chunk, thr = _CHUNK, _copy_threads()
    hst = None if st is None else st._st   # the copy hashes the chunk as it drains it
    _drain_chunks(t.view(-1), [(lo, min(n, lo + chunk), None) for lo in range(0, n, chunk)], side, chunk,
                  lambda p, lo, hi: lib().lz4m_host_copy(dst + lo, p, hi - lo, thr, hst))
    return (out, st.digest()) if st is not None else out


def host_copy_many(dsts, srcs, lens) -> None:
    """dsts[i] <- srcs[i], lens[i] bytes each (host addresses), over the copy
    pool (include/lz4m.h lz4m_host_copy_many)."""
    n = len(lens)
    if n == 0:
        return
    D = (C.c_void_p * n)(*dsts)
    S = (C.c_void_p * n)(*srcs)
    L = (C.c_size_t * n)(*lens)
    lib().lz4m_host_copy_many(D, S, L, n, _copy_threads())

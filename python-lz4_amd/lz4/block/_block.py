"""``lz4.block`` on the MI355X codec.

Drop-in for the reference CPython extension ``lz4/block/_block.c``: same
function names, argument handling, return types, size header and exception
messages (``_block.c:127-400``).  Every call runs the HIP kernels of
``_lz4m.so``; single calls pay one H2D + launch + D2H, so the batched
entry points (``compress_batch`` / ``decompress_batch`` on device tensors,
``compress_many`` / ``decompress_many`` on host buffers) are the throughput
path.  The three compression calls share ``resolve_parse`` (arguments -> one
parse description, or the argument error) and ``_native.launch_blocks`` (the
launch that description names), as the frame calls do.
"""
from __future__ import annotations

import ctypes as C
import operator
import threading

import numpy as np
import torch

from .. import _native as N

INT_MAX = 2**31 - 1
INT_MIN = -(2**31)
_HDR = 4   # _block.c:82, LE32 uncompressed size prefix

# lz4hc.h:47-50, exported by _block.c:508-511
HC_LEVEL_MIN = 3
HC_LEVEL_DEFAULT = 9
HC_LEVEL_OPT_MIN = 10
HC_LEVEL_MAX = 12


class LZ4BlockError(Exception):
    """Call to LZ4 library failed."""


LZ4BlockError.__module__ = "_block"


# -------------------------------------------------------------- arg helpers
def _c_int(value, name: str) -> int:
    """PyArg 'i' conversion: __index__ required, C int range enforced."""
    try:
        v = operator.index(value)
    except TypeError:
        raise TypeError(f"'{type(value).__name__}' object cannot be interpreted as an integer") from None
    if v > INT_MAX:
        raise OverflowError("signed integer is greater than maximum")
    if v < INT_MIN:
        raise OverflowError("signed integer is less than minimum")
    return v


def _buffer(obj, name: str = "source") -> memoryview:
    """PyArg 'y*' conversion: any contiguous buffer; str is rejected."""
    if isinstance(obj, str):
        raise TypeError(f"a bytes-like object is required, not '{type(obj).__name__}'")
    mv = memoryview(obj)
    if not mv.c_contiguous:
        raise BufferError("memoryview: underlying buffer is not C-contiguous")
    return mv.cast("B") if mv.format != "B" or mv.ndim != 1 else mv


def _cap_and_skip(view: memoryview, uncompressed_size: int):
    """(output capacity, leading bytes that are not the block) of a
    decompress source (``_block.c:321-349``): ``uncompressed_size >= 0`` is
    the capacity and the whole source the block, else a LE32 size header
    leads it."""
    if uncompressed_size >= 0:
        return uncompressed_size, 0
    if view.nbytes < _HDR:
        raise ValueError("Input source data size too small")
    cap = int.from_bytes(view[:4], "little")
    if cap > INT_MAX:
        raise ValueError(f"Invalid size: 0x{cap}")
    return cap, _HDR


def _decode_error(status: int, cap: int, from_header: bool):
    """The reference's exception for a decoder status (``_block.c:365-380``),
    None for a good one; a size from the header must be met exactly."""
    if status < 0:
        return LZ4BlockError("Decompression failed: corrupt input or insufficient space in destination buffer. "
                             f"Error code: {-status}")
    if from_header and status != cap:
        return LZ4BlockError(f"Decompressor wrote {status} bytes, but {cap} bytes expected from header")
    return None


def _excl_offsets(lens) -> np.ndarray:
    """int64 start offsets of items of these lengths laid back to back."""
    out = np.zeros(len(lens), np.int64)
    np.cumsum(lens[:-1], dtype=np.int64, out=out[1:])
    return out


def _i64(vals, dev) -> torch.Tensor:
    return torch.tensor(vals, dtype=torch.int64, device=dev)


def _i32(vals, dev) -> torch.Tensor:
    return torch.tensor(vals, dtype=torch.int32, device=dev)


# ------------------------------------------------------------ single calls
def compress(source, mode="default", store_size=True, acceleration=1, compression=9,
             return_bytearray=False, dict=None):
    """compress(source, mode='default', acceleration=1, compression=0, return_bytearray=False)

    Compress source into one LZ4 block (``_block.c:127-271``), output
    byte-identical to the reference: ``lz4.block.compress`` resets an
    ``LZ4_stream_t`` and calls ``LZ4_compress_fast_continue`` (byU32 table,
    hash5), which ``TABLE_U32_HASH5`` reproduces.  With ``dict`` (any
    length, even empty) the stream is first loaded with ``LZ4_loadDict``
    (``_block.c:101-104``, ``lz4.c:1541-1581``) -- lz4m_compress_dict_batch.

    ``mode='high_compression'`` (``_block.c:112-119``) runs the device's
    hash-chain compressor at level ``compression`` (lz4m_compress_hc_batch):
    a valid block near the size of ``LZ4_compress_HC`` at that level, NOT
    byte-identical to it.  Levels below 1 mean 9; levels 10-12 and above
    search as level 9 (``mode='optimal'`` is the higher-ratio parse).  HC with
    ``dict=`` (``LZ4_loadDictHC``) raises ``NotImplementedError`` from this
    call; ``compress_many(mode='high_compression', dict=D)`` and
    ``compress_batch(dict_len=)`` compress with a dictionary.

    ``mode='optimal'`` (not in the reference's binding) runs the device's
    price-based optimal parse searching as level ``compression``
    (lz4m_compress_opt_batch): at level 9 a valid block within 1 % of
    ``LZ4_compress_HC`` at level 12, NOT byte-identical to it.  ``dict=``
    raises ``NotImplementedError``: the optimal parse takes no dictionary.
    """
    src = _buffer(source)
    acceleration = _c_int(acceleration, "acceleration")
    compression = _c_int(compression, "compression")
    if src.nbytes > INT_MAX:
        raise OverflowError("Input too large for LZ4 API")
    d = None
    if dict is not None:
        d = _buffer(dict, "dict")
        if d.nbytes > INT_MAX:
            raise OverflowError("Dictionary too large for LZ4 API")
    p = resolve_parse(mode, accel=acceleration, compression=compression, dict=d, single=True)
    if p.launcher == "table" and d is None:   # one call: lz4m_compress_block_api (one launch on mapped pinned staging)
        N.require_device()
        n = src.nbytes
        hdr = _HDR if store_size else 0
        ptr = C.c_void_p()
        # the output (after the size header) stays in the thread's pinned buffer: one copy into the result
        r = N.lib().lz4m_compress_block_api_staged(N.host_addr(src), n, max(N.compress_bound(n), 1), p.accel, hdr,
                                                   C.byref(ptr))
        if r <= 0:
            raise LZ4BlockError("Compression failed")
        out = C.string_at(ptr.value, hdr + r)
        return bytearray(out) if return_bytearray else out
    if p.launcher != "table":
        how = {"mode": mode, "compression": compression}
    else:
        # dictionary memory that ends where the source begins: the reference's
        # LZ4_compress_fast_continue sees dictEnd == source and takes prefix mode
        # (lz4.c:1671-1676; LZ4_loadDict keeps no dictionary below 8 bytes)
        prefix = d.nbytes >= 8 and src.nbytes > 0 and N.host_addr(d) + d.nbytes == N.host_addr(src)
        how = {"accel": p.accel, "dict": d, "dict_prefix": prefix}
    out = compress_many([src], store_size=bool(store_size), as_bytearray=bool(return_bytearray), **how)[0]
    if out is None:
        raise LZ4BlockError("Compression failed")
    return out


def decompress(source, uncompressed_size=-1, return_bytearray=False, dict=None):
    """decompress(source, uncompressed_size=-1, return_bytearray=False)

    Decompress one LZ4 block (``_block.c:273-400``).  With
    ``uncompressed_size >= 0`` the whole source is the block and the value is
    a capacity; otherwise a LE32 size header leads the block and the decoded
    size must equal it.
    """
    src = _buffer(source)
    uncompressed_size = _c_int(uncompressed_size, "uncompressed_size")
    if src.nbytes > INT_MAX:
        raise OverflowError("Input too large for LZ4 API")
    dview = None
    if dict is not None:
        dview = _buffer(dict, "dict")
        if dview.nbytes > INT_MAX:
            raise OverflowError("Dictionary too large for LZ4 API")
    if dview is None or not dview.nbytes:   # one call: lz4m_decompress_safe
        N.require_device()
        cap, skip = _cap_and_skip(src, uncompressed_size)
        sp = N.host_addr(src)
        p = C.c_void_p()
        # the output stays in the thread's pinned buffer: one copy into the result
        r = N.lib().lz4m_decompress_safe_staged(None if sp is None else sp + skip, src.nbytes - skip, cap, C.byref(p))
        err = _decode_error(r, cap, uncompressed_size < 0)
        if err is not None:
            raise err
        out = C.string_at(p.value, r) if r else b""
        return bytearray(out) if return_bytearray else out
    res = decompress_many([src], uncompressed_size=uncompressed_size, dict=dview,
                          as_bytearray=bool(return_bytearray), raise_errors=True)
    return res[0]


# ---------------------------------------------------- host-buffer batches
# A call from host memory moves everything through one pinned staging buffer
# per thread and device: block table + payload in ONE host-to-device copy,
# status/lengths + output in ONE device-to-host copy (the reference does one
# malloc + memcpy per call, _block.c:215, :256-263; a launch per small tensor
# would dominate a 64 KiB call).
_tls = threading.local()
_ALIGN = 256


def _al(x: int) -> int:
    return (x + _ALIGN - 1) // _ALIGN * _ALIGN


def _stage(dev, host_bytes: int, dev_bytes: int):
    """(pinned host uint8, device uint8) buffers of at least these sizes,
    cached per thread and device, grown geometrically."""
    cache = getattr(_tls, "stage", None)
    if cache is None:
        cache = _tls.stage = {}
    h, d = cache.get(dev, (None, None))
    if h is None or h.numel() < host_bytes:
        h = torch.empty(max(host_bytes, 2 * (h.numel() if h is not None else 0), 1 << 20), dtype=torch.uint8,
                        pin_memory=True)
    if d is None or d.numel() < dev_bytes:
        d = torch.empty(max(dev_bytes, 2 * (d.numel() if d is not None else 0), 1 << 20), dtype=torch.uint8,
                        device=dev)
    cache[dev] = (h, d)
    return h, d


class _Layout:
    """Byte layout of one staged batch: n-entry tables, then payload, then
    (device only) the n-entry result table and the output region."""

    def __init__(self, n: int, payload: int, out_bytes: int):
        self.src_off = 0
        self.src_len = _al(8 * n)
        self.dst_off = self.src_len + _al(4 * n)
        self.dst_cap = self.dst_off + _al(8 * n)
        self.payload = self.dst_cap + _al(4 * n)
        self.h2d = self.payload + payload                  # bytes copied in
        self.result = _al(self.h2d)
        self.out = self.result + _al(4 * n)
        self.total = self.out + max(out_bytes, 1)            # device bytes
        self.d2h = self.total - self.result                  # bytes copied out


def _stage_in(dev, views, offs, lens, d_off, caps, skip=None):
    """Stage tables + packed payload, copy them to the device in one go;
    returns (layout, host, device) with the device views ready to launch on.
    ``views`` are packed back to back; ``offs``/``lens`` (one per block) say
    where the blocks are in that payload."""
    n = len(offs)
    payload = sum(v.nbytes for v in views)
    lay = _Layout(n, payload, sum(caps))
    h, d = _stage(dev, lay.total, lay.total)
    hn = h.numpy()
    hn[lay.src_off:lay.src_off + 8 * n].view(np.int64)[:] = offs if skip is None else np.add(offs, skip)
    hn[lay.src_len:lay.src_len + 4 * n].view(np.int32)[:] = lens if skip is None else np.subtract(lens, skip)
    hn[lay.dst_off:lay.dst_off + 8 * n].view(np.int64)[:] = d_off
    hn[lay.dst_cap:lay.dst_cap + 4 * n].view(np.int32)[:] = caps
    pos = lay.payload
    if len(views) >= _MANY and payload >= _MANY_BYTES:   # one pooled native copy of every block
        base = h.data_ptr()
        dsts, srcs, ns = [], [], []
        for v in views:
            dsts.append(base + pos)
            srcs.append(N.host_addr(v))
            ns.append(v.nbytes)
            pos += v.nbytes
        N.host_copy_many(dsts, srcs, ns)
    else:
        for v in views:
            hn[pos:pos + v.nbytes] = np.frombuffer(v, dtype=np.uint8)
            pos += v.nbytes
    d[:lay.h2d].copy_(h[:lay.h2d], non_blocking=True)
    return lay, h, d


# batches of at least this many blocks and bytes pack and unpack through one
# pooled native copy (lz4m_host_copy_many) instead of a numpy copy per block
_MANY, _MANY_BYTES = 32, 4 << 20


def _results_many(host, d_off, sizes, hdr_lens, as_bytearray):
    """New bytes (or bytearrays) for blocks of sizes[i] >= 0 bytes at host
    offset d_off[i] (None where sizes[i] < 0), prefixed with the LE32 of
    hdr_lens[i] when hdr_lens is given; filled by one pooled copy."""
    base = host.ctypes.data
    res, dsts, srcs, ns = [], [], [], []
    for i, L in enumerate(sizes):
        if L < 0:
            res.append(None)
            continue
        hdr = 4 if hdr_lens is not None else 0
        b, addr = N._new_host_buffer(hdr + L, as_bytearray) if hdr + L else ((bytearray() if as_bytearray else b""), 0)
        if hdr:
            C.memmove(addr, hdr_lens[i].to_bytes(4, "little"), 4)
        if L:
            dsts.append(addr + hdr)
            srcs.append(base + int(d_off[i]))
            ns.append(L)
        res.append(b)
    N.host_copy_many(dsts, srcs, ns)
    return res


def _dev_views(lay: _Layout, d: torch.Tensor, n: int):
    def sl(a, nb, dt):
        return d[a:a + nb].view(dt)
    return (sl(lay.payload, max(lay.h2d - lay.payload, 1), torch.uint8), sl(lay.src_off, 8 * n, torch.int64),
            sl(lay.src_len, 4 * n, torch.int32), d[lay.out:lay.total], sl(lay.dst_off, 8 * n, torch.int64),
            sl(lay.dst_cap, 4 * n, torch.int32), sl(lay.result, 4 * n, torch.int32))


def _stage_out(lay: _Layout, h: torch.Tensor, d: torch.Tensor, n: int):
    """One device-to-host copy of the result table + output region."""
    h[lay.result:lay.total].copy_(d[lay.result:lay.total], non_blocking=True)
    torch.cuda.current_stream(d.device).synchronize()
    hn = h.numpy()
    return hn[lay.result:lay.result + 4 * n].view(np.int32).tolist(), hn[lay.out:lay.total]


_DICT_WINDOW = 65536   # the bytes of a dictionary an LZ4 block can reach


class PreparedDict:
    """A dictionary made ready for the parallel parse (``prepare_dict``):
    ``tail``, the device copy of its last 64 KiB; ``dict_len``, its full
    length; ``table``, the 8 KiB hash table of the tail
    (lz4m_pcompress_dict_prepare).  Hashed once, used by any number of
    ``compress_batch(dict_buf=)`` / ``compress_many(dict=)`` calls; the blocks
    decode with the dictionary's bytes (``decompress_many(dict=)``,
    ``decompress_batch(dict_buf=prepared.tail)``)."""

    __slots__ = ("tail", "dict_len", "table")

    def __init__(self, tail: torch.Tensor, dict_len: int, table: torch.Tensor):
        self.tail, self.dict_len, self.table = tail, dict_len, table


def _prepare_dict(d, stream=None, copy: bool = True) -> PreparedDict:
    if isinstance(d, PreparedDict):
        return d
    if isinstance(d, torch.Tensor):
        if d.dtype != torch.uint8 or d.dim() != 1 or not d.is_cuda:
            raise ValueError("a dictionary tensor must be a one-dimensional uint8 device tensor")
        tail = d[max(d.numel() - _DICT_WINDOW, 0):]
        if copy or not tail.is_contiguous():
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(d.device)):
                tail = tail.clone()
        full = d.numel()
    else:
        dv = _buffer(d, "dict")
        full = dv.nbytes
        tail = N.to_device(dv[max(full - _DICT_WINDOW, 0):], N.device())
        if stream is not None:   # the upload ran on the current stream
            stream.wait_stream(torch.cuda.current_stream(tail.device))
    return PreparedDict(tail, full, N.pcompress_dict_prepare(tail, stream))


def prepare_dict(dict, stream=None) -> PreparedDict:
    """Upload (a host buffer) or copy (a uint8 device tensor) the last 64 KiB
    of ``dict`` and hash them, once, for ``compress_batch(table=PARSE_PARALLEL,
    dict_buf=)`` and ``compress_many(dict=, table=PARSE_PARALLEL)``.  Stream-
    ordered on ``stream`` (default: the current one)."""
    return _prepare_dict(dict, stream)


_TABLES = {"block": N.TABLE_U32_HASH5, "default": N.TABLE_AUTO, "u16": N.TABLE_U16_HASH4}
_MODES = {False: ("default", "high_compression", "optimal"), True: ("default", "fast", "high_compression", "optimal")}


def resolve_parse(mode="default", *, accel=1, compression=9, table=N.TABLE_U32_HASH5, dict=None,
                  dict_prefix=False, dict_len=None, dict_buf=None, single=False) -> N.Parse:
    """The parse the arguments of ``compress`` (``single``: the reference's
    mode names, no HC dictionary), ``compress_many`` or ``compress_batch`` ask
    for, as the description ``N.launch_blocks`` takes, or the call's exception
    for arguments that do not go together.  Pure: no data, no launch."""
    if single and not isinstance(mode, str):
        raise TypeError(f"compress() argument 'mode' must be str, not {type(mode).__name__}")
    if mode not in _MODES[single]:
        names = "standard, fast, high_compression, optimal" if single else "default, high_compression, optimal"
        raise ValueError(f"Invalid mode argument: {mode}. Must be one of: {names}")
    if mode == "optimal":
        if dict is not None or dict_len is not None or dict_buf is not None:
            raise NotImplementedError("mode='optimal' with a dictionary (dict= / dict_len=) is not built: the optimal "
                                      "parse has no history; use mode='high_compression' with a dictionary")
        return N.Parse("opt", level=_c_int(compression, "compression"))
    if mode == "high_compression" and single and dict is not None:
        raise NotImplementedError(
            "mode='high_compression' with dict= (LZ4_loadDictHC) is not built on the MI355X codec; "
            "compress without a dictionary, or use mode='default' or mode='fast' with dict=")
    level = _c_int(compression, "compression")
    hc = mode == "high_compression"
    shared = dict is not None and not hc and not dict_prefix and table == N.PARSE_PARALLEL
    if isinstance(dict, PreparedDict) and not shared:
        raise ValueError("a PreparedDict is only valid with table=PARSE_PARALLEL, mode='default' and no dict_prefix")
    if dict_buf is not None:
        if hc:
            raise ValueError("dict_buf is not valid with mode='high_compression' (use dict_len)")
        if dict_len is not None:
            raise ValueError("dict_buf (one shared dictionary) and dict_len (one per block) exclude each other")
        if table != N.PARSE_PARALLEL:
            raise ValueError("dict_buf is only valid with table=PARSE_PARALLEL")
        shared = True
    if dict_len is not None and not hc:
        raise ValueError("dict_len is only valid with mode='high_compression'")
    history = "shared" if shared else "hist" if dict is not None or dict_len is not None else ""
    if hc:
        return N.Parse("hc", level=level, history=history)
    accel = 1 if single and mode == "default" else int(accel)
    if history == "shared":
        return N.Parse("table", N.PARSE_PARALLEL, history=history)
    if history == "hist":   # the dictionary compressor has one table, lz4.block.compress's
        return N.Parse("table", N.TABLE_U32_HASH5, accel, history=history, prefix=bool(dict_prefix))
    return N.Parse("table", int(_TABLES.get(table, table)), accel)


def compress_many(blocks, accel: int = 1, store_size: bool = True, as_bytearray: bool = False,
                  table: int = N.TABLE_U32_HASH5, dict=None, dict_prefix: bool = False,
                  mode: str = "default", compression: int = 9):
    """Compress a sequence of host buffers as independent blocks in one
    launch.  Returns a list of bytes (None for a block that failed, i.e.
    input larger than LZ4_MAX_INPUT_SIZE).  ``dict`` (a buffer, possibly
    empty): every block is compressed as lz4.block.compress(dict=dict) does;
    the dictionary's last 64 KiB are staged in front of each block.
    ``dict_prefix``: compress as the reference does when the dictionary's
    memory ends where each source begins (prefix mode, lz4.c:1671).
    ``mode="high_compression"``: the hash-chain compressor at level
    ``compression`` (valid blocks near LZ4_compress_HC's size, not
    byte-identical; ``accel``, ``table`` and ``dict_prefix`` are ignored).
    With ``dict`` of any length (lz4m_compress_hc_dict_batch) matches may
    reach into the dictionary's last 64 KiB, and the result decodes with
    ``lz4.block.decompress(comp, dict=dict)``; an empty ``dict`` gives the
    bytes of no ``dict``.
    ``mode="optimal"``: the price-based optimal parse searching as level
    ``compression`` (lz4m_compress_opt_batch); ``dict`` raises
    ``NotImplementedError``.
    ``dict`` with ``table=PARSE_PARALLEL`` (mode "default", no
    ``dict_prefix``): the parallel parse with the dictionary as every block's
    history (lz4m_pcompress_dict_batch): blocks up to 64 KiB, valid blocks
    that decode with ``dict=dict``, not byte-identical to the exact parse.
    The dictionary is uploaded and hashed once per call -- not staged with
    every block -- or not at all when ``dict`` is a ``PreparedDict``
    (``prepare_dict``), which only this combination accepts."""
    p = resolve_parse(mode, accel=accel, compression=compression, table=table, dict=dict, dict_prefix=dict_prefix)
    staged = p.history == "hist"   # the dictionary's last 64 KiB are staged in front of each block
    views = [_buffer(b) for b in blocks]
    dev = N.device()
    n = len(views)
    if n == 0:
        return []
    lens = [v.nbytes for v in views]
    caps = [max(N.compress_bound(L), 1) for L in lens]
    d_off = _excl_offsets(caps)
    extra = None
    if not staged:
        offs = _excl_offsets(lens)
        payload = views
        if p.history == "shared":
            extra = _prepare_dict(dict)
    else:
        dv = _buffer(dict, "dict")
        # LZ4_loadDict keeps the last 64 KiB (lz4.c:1568) and nothing of a dictionary below 8 bytes; HC keeps any
        small = dv.nbytes < 8 and p.launcher != "hc"
        tail = dv[:0] if small else dv[-65536:]
        t = tail.nbytes
        offs = np.arange(1, n + 1, dtype=np.int64) * t + _excl_offsets(lens)
        payload = [x for v in views for x in (tail, v)]
        extra = torch.full((n,), dv.nbytes, dtype=torch.int32, device=dev)
        p = p._replace(prefix=p.prefix and not small)
    lay, h, d = _stage_in(dev, payload, offs, lens, d_off, caps)
    # (with max_len the parallel parse's large-block launch is the segmented one: the frame calls' choice only)
    N.launch_blocks(p, *_dev_views(lay, d, n), n, extra=extra, max_len=None if p.launcher == "table" else max(lens))
    olen, host = _stage_out(lay, h, d, n)
    if n >= _MANY and sum(L for L in olen if L > 0) >= _MANY_BYTES:
        return _results_many(host, d_off, [L if L > 0 else -1 for L in olen], lens if store_size else None,
                             as_bytearray)
    res = []
    for i in range(n):
        L = olen[i]
        if L <= 0:
            res.append(None)
            continue
        o = int(d_off[i])
        body = host[o:o + L].tobytes()
        if store_size:
            body = lens[i].to_bytes(4, "little") + body
        res.append(bytearray(body) if as_bytearray else body)
    return res


def _restage_caps(dev, lay: _Layout, h, d, n: int, d_off, caps):
    """A staged batch whose capacities are known only now: the layout with
    an output region of sum(caps) bytes, the staged tables and payload kept
    on the device (moved when the buffer has to grow) and the two output
    tables written again.  Returns (layout, host, device)."""
    lay2 = _Layout(n, lay.h2d - lay.payload, sum(caps))
    h2, d2 = _stage(dev, lay2.total, lay2.total)
    if d2 is not d:
        d2[:lay.h2d].copy_(d[:lay.h2d])
    hn = h2.numpy()
    hn[lay2.dst_off:lay2.dst_off + 8 * n].view(np.int64)[:] = d_off
    hn[lay2.dst_cap:lay2.dst_cap + 4 * n].view(np.int32)[:] = caps
    d2[lay2.dst_off:lay2.payload].copy_(h2[lay2.dst_off:lay2.payload], non_blocking=True)
    return lay2, h2, d2


def _dict_args(dict, n: int, dev):
    """(device dictionary, its offsets, its lengths) shared by n blocks, or
    three Nones without a dictionary (an empty one is none)."""
    if dict is None or not _buffer(dict).nbytes:
        return None, None, None
    dv = _buffer(dict)
    return (N.to_device(dv, dev), torch.zeros(n, dtype=torch.int64, device=dev),
            torch.full((n,), dv.nbytes, dtype=torch.int32, device=dev))


def decompress_many(blocks, uncompressed_size=-1, dict=None, as_bytearray: bool = False,
                    raise_errors: bool = True):
    """Decompress a sequence of host buffers in one launch.

    ``uncompressed_size`` is one value for all blocks or a list: an int >= 0
    is the block's capacity, a negative int means "read the LE32 size
    header", and ``None`` means "no size header and the size is unknown"
    (``compress(store_size=False)`` output, raw ``LZ4_compress_*`` output).
    For the ``None`` blocks the staged sources first go through the decoded-
    size pass (``decompressed_size_batch``, with ``dict``'s length), one
    read-back of the sizes lays the output out, and each decodes at exactly
    its size (see ``decompress_batch`` for what that capacity means).  With
    ``raise_errors`` the first failing block raises the reference's
    exception; otherwise failing blocks yield the LZ4BlockError instance in
    their slot.
    """
    views = [_buffer(b) for b in blocks]
    n = len(views)
    if n == 0:
        return []
    sizes = list(uncompressed_size) if isinstance(uncompressed_size, (list, tuple)) else [uncompressed_size] * n
    unknown = [us is None for us in sizes]
    caps, skip, errors = [], [], [None] * n
    for i, (v, us) in enumerate(zip(views, sizes)):
        if us is None:   # capacity from the size pass, below
            caps.append(0)
            skip.append(0)
            continue
        try:
            cap, sk = _cap_and_skip(v, us)
        except ValueError as err:
            if raise_errors:
                raise
            errors[i], cap, sk = err, 0, 0   # decoded as an empty block, reported in its slot
        caps.append(cap)
        skip.append(sk)
    from_header = [us is not None and us < 0 for us in sizes]
    dev = N.device()
    lens = [v.nbytes for v in views]
    offs = _excl_offsets(lens)
    d_off = _excl_offsets(caps)
    lay, h, d = _stage_in(dev, views, offs, lens, d_off, caps, skip=skip)
    d_dict, dict_off, dict_len = _dict_args(dict, n, dev)
    passed = None
    if any(unknown):
        d_src, src_off, src_len = _dev_views(lay, d, n)[:3]
        size = torch.empty(n, dtype=torch.int32, device=dev)
        N.launch_decompressed_size(d_src, src_off, src_len, size, n, dict_len=dict_len)
        passed = size.tolist()   # the one read-back that lays the output out
        caps = [max(p, 0) if u else c for p, u, c in zip(passed, unknown, caps)]
        d_off = _excl_offsets(caps)
        lay, h, d = _restage_caps(dev, lay, h, d, n, d_off, caps)
    d_src, src_off, src_len, d_dst, dst_off, dst_cap, status = _dev_views(lay, d, n)
    if d_dict is not None:
        N.launch_decompress(d_src, src_off, src_len, d_dst, dst_off, dst_cap, status, n,
                            dict_buf=d_dict, dict_off=dict_off, dict_len=dict_len)
    else:
        N.launch_decompress(d_src, src_off, src_len, d_dst, dst_off, dst_cap, status, n,
                            src_bytes=int(sum(lens)))
    st, host = _stage_out(lay, h, d, n)
    if passed is not None:   # a block the size pass rejected keeps that status
        st = [p if u and p < 0 else r for r, p, u in zip(st, passed, unknown)]
    if n >= _MANY and all(e is None for e in errors) and all(
            r >= 0 and (r == c or not fh) for r, c, fh in zip(st, caps, from_header)) and sum(st) >= _MANY_BYTES:
        return _results_many(host, d_off, st, None, as_bytearray)   # every block decoded as asked
    res = []
    for i in range(n):
        if errors[i] is not None:
            res.append(errors[i])
            continue
        r = st[i]
        err = _decode_error(r, caps[i], from_header[i])
        if err is not None:
            if raise_errors:
                raise err
            res.append(err)
            continue
        o = int(d_off[i])
        body = host[o:o + r].tobytes() if r else b""
        res.append(bytearray(body) if as_bytearray else body)
    return res


def decompressed_size_many(blocks, dict=None, raise_errors: bool = True):
    """The decoded size of each host buffer (a block without a size header),
    without decoding it: ``decompressed_size_batch`` on the staged blocks,
    with ``dict``'s length as every block's dictionary length.  A block the
    pass rejects raises ``LZ4BlockError`` ("Decompression failed ..."); with
    ``raise_errors=False`` its negative status stays in the list."""
    views = [_buffer(b) for b in blocks]
    n = len(views)
    if n == 0:
        return []
    dev = N.device()
    lens = [v.nbytes for v in views]
    zeros = [0] * n
    lay, _h, d = _stage_in(dev, views, _excl_offsets(lens), lens, zeros, zeros)
    d_src, src_off, src_len = _dev_views(lay, d, n)[:3]
    nd = 0 if dict is None else _buffer(dict).nbytes
    dict_len = torch.full((n,), nd, dtype=torch.int32, device=dev) if nd else None
    size = torch.empty(n, dtype=torch.int32, device=dev)
    N.launch_decompressed_size(d_src, src_off, src_len, size, n, dict_len=dict_len)
    out = size.tolist()
    if raise_errors:
        for r in out:
            if r < 0:
                raise _decode_error(r, 0, False)
    return out


# ------------------------------------------------- device-resident batches
def compress_batch(src: torch.Tensor, src_off: torch.Tensor, src_len: torch.Tensor, *,
                   table: str | int = "block", acceleration: int = 1, dst: torch.Tensor | None = None,
                   dst_off: torch.Tensor | None = None, dst_cap: torch.Tensor | None = None, stream=None,
                   mode: str = "default", compression: int = 9, dict_len: torch.Tensor | None = None,
                   dict_buf: "PreparedDict | torch.Tensor | None" = None):
    """Compress n device-resident blocks in one stream-ordered launch.

    ``src`` uint8 (HBM), ``src_off`` int64[n], ``src_len`` int32[n].
    ``table``: "block" (lz4.block.compress parse, byU32/hash5), "default"
    (LZ4_compress_default's choice by size; byU16/hash4 below 65547 B) or a
    TABLE_* constant.  Output slots default to LZ4_compressBound(len) each.
    Returns (dst, dst_off, out_len) with out_len int32[n] (0 = did not fit).
    No host synchronisation.

    ``mode="high_compression"``: the hash-chain (HC) compressor at level
    ``compression`` instead (lz4m_compress_hc_batch; ``table`` and
    ``acceleration`` are ignored): valid blocks near the size of
    LZ4_compress_HC at that level, NOT byte-identical to it.  Levels below 1
    mean 9, 3..9 search 4..256 chain candidates per position, levels 10-12
    and above search as 9 (``mode="optimal"`` is the higher-ratio parse).  A
    block that does not fit its slot reports 0; an exact fit is accepted.
    ``dict_len`` int32[n] (this mode only, lz4m_compress_hc_dict_batch):
    block i has a dictionary of dict_len[i] bytes whose last min(dict_len[i],
    65536) bytes lie immediately before it in ``src``; matches may reach into
    them, and the block decodes with those bytes as its dictionary.
    dict_len[i] <= 0: no dictionary.

    ``mode="optimal"``: the price-based optimal parse searching as level
    ``compression`` (lz4m_compress_opt_batch): at level 9 within 1 % of
    LZ4_compress_HC(12), NOT byte-identical.  Its workspace grows with the
    longest block, so this mode reads ``src_len.max()`` back: one host
    synchronisation.  ``dict_len`` / ``dict_buf`` raise NotImplementedError.

    ``dict_buf`` (``table=PARSE_PARALLEL`` only, lz4m_pcompress_dict_batch):
    the one dictionary of all blocks, the counterpart of
    ``decompress_batch(dict_buf=)``: a ``PreparedDict`` (``prepare_dict``), or
    a uint8 device tensor, which is hashed on the spot on the call's stream
    (neither is copied per block).  Matches may reach into its last 64 KiB;
    the blocks (up to 64 KiB each) decode with it as their dictionary.  Below
    4 bytes it changes nothing.
    """
    p = resolve_parse(mode, accel=acceleration, compression=compression, table=table, dict_len=dict_len,
                      dict_buf=dict_buf)
    n = src_off.numel()
    dev = src.device
    if dst_cap is None:
        dst_cap = (src_len.to(torch.int64) + src_len.to(torch.int64) // 255 + 16).to(torch.int32)
    if dst_off is None:
        dst_off = N.exclusive_scan(dst_cap, stream=stream)[:n]
    if dst is None:
        total = int((dst_off[-1] + dst_cap[-1]).item()) if n else 1
        dst = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        extra = None
        if p.history == "shared":
            extra = _prepare_dict(dict_buf, stream, copy=False)
        elif p.history == "hist":
            extra = dict_len.to(torch.int32)
        N.launch_blocks(p, src, src_off, src_len, dst, dst_off, dst_cap, out_len, n, extra=extra, stream=stream)
    return dst, dst_off, out_len


def decompressed_size_batch(src: torch.Tensor, src_off: torch.Tensor, src_len: torch.Tensor, *,
                            dict_len: torch.Tensor | None = None, walk: str = "auto", stream=None):
    """The decoded sizes of n device-resident blocks without decoding them,
    one stream-ordered launch (lz4m_decompressed_size_batch), no host
    synchronisation.  Returns int32[n]: what ``decompress_batch`` reports for
    block i at a capacity large enough not to matter (any capacity of at
    least 255 * src_len[i] + 64 gives it) -- the decoded size, or -(pos)-1
    with the reference's error position.  ``dict_len`` int32[n]: the length of
    each block's dictionary (matches may reach that far before the block;
    only the length counts).  A size above 2**31 - 1 reports -2**31.
    ``walk``: "lane" (a lane per block, large batches), "wave" (a wavefront
    per block, few or large blocks) or "auto" (by batch size); all give the
    same values.  Validates a batch of untrusted blocks for everything but
    the bytes a match copies."""
    n = src_off.numel()
    size = torch.empty(n, dtype=torch.int32, device=src.device)
    N.launch_decompressed_size(src, src_off, src_len, size, n, stream, dict_len, walk)
    return size


def decompress_batch(src: torch.Tensor, src_off: torch.Tensor, src_len: torch.Tensor,
                     dst_cap: torch.Tensor | None = None, *,
                     dst: torch.Tensor | None = None, dst_off: torch.Tensor | None = None,
                     dict_buf: torch.Tensor | None = None, dict_off: torch.Tensor | None = None,
                     dict_len: torch.Tensor | None = None, stream=None):
    """Decompress n device-resident blocks in one stream-ordered launch.

    Returns (dst, dst_off, status): status int32[n] is the decoded size or
    -(pos)-1 exactly as LZ4_decompress_safe(_usingDict) would return.

    ``dst_cap=None``: the sizes are not known.  They come from the decoded-
    size pass (``decompressed_size_batch``, with ``dict_len`` when a
    dictionary is given): dst_cap = size.clamp(min=0), ``dst_off`` its
    exclusive scan, and the output is exactly packed (one read-back for the
    total, as ``dst=None`` always costs).  ``status`` is what the decode
    returns at that capacity:
      - a block that decodes only with slack fails here: one whose last match
        starts within 12 bytes of the end of the output or ends within 5
        (lz4.c:2296, :2312).  No conformant compressor writes such blocks, and
        the reference fails at the same capacity;
      - a block whose size pass failed has capacity 0 and keeps the size
        pass's negative status.
    """
    n = src_off.numel()
    dev = src.device
    passed = None
    if dst_cap is None:
        passed = decompressed_size_batch(src, src_off, src_len, dict_len=None if dict_buf is None else dict_len,
                                         stream=stream)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            dst_cap = passed.clamp(min=0)
    if dst_off is None:
        dst_off = N.exclusive_scan(dst_cap, stream=stream)[:n]
    if dst is None:
        total = int((dst_off[-1] + dst_cap[-1]).item()) if n else 1
        dst = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    N.launch_decompress(src, src_off, src_len, dst, dst_off, dst_cap, status, n, stream,
                        dict_buf, dict_off, dict_len)
    if passed is not None:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            status = torch.where(passed < 0, passed, status)
    return dst, dst_off, status


def compact(buf: torch.Tensor, off: torch.Tensor, length: torch.Tensor, stream=None):
    """Pack variable-length items (e.g. compress_batch output) contiguously:
    returns (packed uint8, offsets int64[n+1])."""
    n = off.numel()
    offs = N.exclusive_scan(length, stream=stream)
    total = int(offs[-1].item())
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=buf.device)
    N.gather(buf, off, length, out, offs, n, stream)
    return out[:total], offs


def xxh32_batch(src: torch.Tensor, off: torch.Tensor, length: torch.Tensor, seed: int = 0, stream=None):
    """XXH32 of n device-resident items (uint32[n] as int64 tensor view)."""
    n = off.numel()
    out = torch.empty(n, dtype=torch.int32, device=src.device)
    N.launch_xxh32_batch(src, off, length.to(torch.int64), seed, out, n, stream)
    return out


def decompress_host(comp: torch.Tensor, comp_off: torch.Tensor, comp_len: torch.Tensor, out: torch.Tensor,
                    out_off: torch.Tensor, out_cap: torch.Tensor, *, chunk_blocks: int = 16384,
                    device=None) -> torch.Tensor:
    """Decode n blocks that start and end in HOST memory (a file's or
    socket's bytes), pipelined over PCIe: chunk i+1 is copied in while
    chunk i decodes and chunk i-1 is copied out (three HIP streams, two
    device buffer sets).  comp / out are uint8 host tensors (pin them for
    the copies to overlap); comp_off / out_off int64, comp_len / out_cap
    int32 host tensors, blocks in increasing position order in both.
    Returns the int32 status of every block (host), as LZ4_decompress_safe
    would return it.  Chunks of 32 768 blocks or more run the large-batch
    row decoder, smaller ones the one-wave-per-block decoder
    (lz4m_decompress_batch_sel's switch-over).  The
    call is bound by the download; smaller chunks start it sooner: 262 144
    silesia-like blocks ran at 42.8 / 45.2 / 46.2 GiB/s with chunks of
    65 536 / 32 768 / 16 384 blocks (the default; profiles/r05/r05at)."""
    dev = device or N.device()
    n = comp_off.numel()
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return status.cpu()
    c_off, c_len = comp_off.to(torch.int64), comp_len.to(torch.int32)
    o_off, o_cap = out_off.to(torch.int64), out_cap.to(torch.int32)
    if bool((c_off[1:] < c_off[:-1] + c_len[:-1]).any()) or bool((o_off[1:] < o_off[:-1] + o_cap[:-1]).any()):
        raise ValueError("blocks must be in increasing, non-overlapping position order")
    chunks = [(lo, min(n, lo + chunk_blocks)) for lo in range(0, n, chunk_blocks)]

    def span(off, ln, lo, hi):
        return int(off[lo]), int(off[hi - 1]) + int(ln[hi - 1])

    in_max = max(b - a for a, b in (span(c_off, c_len, lo, hi) for lo, hi in chunks))
    out_max = max(b - a for a, b in (span(o_off, o_cap, lo, hi) for lo, hi in chunks))
    d_in = [torch.empty(in_max + 16, dtype=torch.uint8, device=dev) for _ in range(2)]
    d_out = [torch.empty(max(out_max, 1), dtype=torch.uint8, device=dev) for _ in range(2)]
    s_in, s_dec, s_out = torch.cuda.Stream(dev), torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    ev_in = [torch.cuda.Event() for _ in range(2)]
    ev_dec = [torch.cuda.Event() for _ in range(2)]
    ev_free = [None, None]
    # every chunk's block offsets, rebased to its buffers, in one upload (a
    # per-chunk upload from pageable memory would block the host thread)
    base_c = torch.zeros(n, dtype=torch.int64)
    base_o = torch.zeros(n, dtype=torch.int64)
    for lo, hi in chunks:
        base_c[lo:hi] = int(c_off[lo])
        base_o[lo:hi] = int(o_off[lo])
    meta = torch.stack([c_off - base_c, o_off - base_o]).to(dev)
    lens = torch.stack([c_len, o_cap]).to(dev)
    cur = torch.cuda.current_stream(dev)
    s_in.wait_stream(cur)
    s_out.wait_stream(cur)
    s_dec.wait_stream(cur)
    try:
        # Copies are queued only once what they wait for is done (the host
        # waits on the event): a copy queued behind an event holds up the
        # copies in the other direction on the copy engine (the upload of
        # chunk i+1 waited for the decode of chunk i, r05ac/r05ad).
        def issue_out(b, b0, b1):
            ev_dec[b].synchronize()                                # its decode is done
            with torch.cuda.stream(s_out):
                out[b0:b1].copy_(d_out[b][: b1 - b0], non_blocking=True)
                ev_free[b] = torch.cuda.Event()
                ev_free[b].record(s_out)

        pending = None
        for i, (lo, hi) in enumerate(chunks):
            b = i & 1
            a0, a1 = span(c_off, c_len, lo, hi)
            if ev_free[b] is not None:
                ev_free[b].synchronize()                           # chunk i-2 has left buffer b
            with torch.cuda.stream(s_in):
                d_in[b][: a1 - a0].copy_(comp[a0:a1], non_blocking=True)
                ev_in[b].record(s_in)
            with torch.cuda.stream(s_dec):
                s_dec.wait_event(ev_in[b])
                N.launch_decompress(d_in[b], meta[0, lo:hi], lens[0, lo:hi], d_out[b], meta[1, lo:hi],
                                    lens[1, lo:hi], status[lo:hi], hi - lo, s_dec)
                ev_dec[b].record(s_dec)
            if pending is not None:
                issue_out(*pending)
            pending = (b,) + span(o_off, o_cap, lo, hi)
        issue_out(*pending)
    finally:
        # (on an error too: no copy or launch may still use the buffers freed on return)
        for s_ in (s_in, s_dec, s_out):
            s_.synchronize()
    cur.wait_stream(s_out)
    cur.wait_stream(s_dec)
    st = status.cpu()
    torch.cuda.synchronize(dev)
    return st

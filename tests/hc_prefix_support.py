"""Shared pieces of tests/test_hc_prefix_model.py and tests/test_gpu_hc_prefix.py:
the CPU model of the HC parse of a block with a prefix
(hc_model_compress_prefix of tests/hc_model/hc_model.c, hc_support's library)
and the (prefix, block) cases both files use."""
import functools

import numpy as np

import hc_support as H

PREFIX_LENGTHS = (1, 3, 4, 7, 8, 63, 64, 65, 4096, 65535, 65536)
BLOCK_LENGTHS = (0, 1, 12, 13, 14, 64, 65, 4096, 65536, 65537)
PREFIX_MAX = 65536
FRAME_BLOCK = 65536          # block_size_id 4
FRAME_OVERHEAD = 15 + 4      # header with the content size, end mark (no checksums); plus 4 per block


def model_compress_at(buf: np.ndarray, start: int, n: int, prefix_len: int, level: int,
                      cap: int | None = None) -> bytes | None:
    """The model's block for buf[start:start + n] with the prefix_len bytes
    before it as history (None when it does not fit ``cap``)."""
    assert 0 <= prefix_len <= min(start, PREFIX_MAX) and start + n <= buf.size
    cap = H.compress_bound(n) if cap is None else cap
    dst = np.zeros(max(cap, 1), dtype=np.uint8)
    r = H.model_lib().hc_model_compress_prefix(buf.ctypes.data + start - prefix_len, prefix_len, n, dst.ctypes.data,
                                               cap, level)
    return None if r <= 0 else dst[:r].tobytes()


def model_compress_prefix(prefix: bytes, block: bytes, level: int, cap: int | None = None) -> bytes | None:
    """The model's block for ``block`` after ``prefix`` (its last 64 KiB count)."""
    prefix = bytes(prefix)[-PREFIX_MAX:]
    buf = np.frombuffer(prefix + bytes(block) + b"\0", dtype=np.uint8)
    return model_compress_at(buf, len(prefix), len(block), len(prefix), level, cap)


@functools.lru_cache(maxsize=None)
def grid_cases() -> tuple:
    """(name, prefix, block) for PREFIX_LENGTHS x BLOCK_LENGTHS x {zeros, a
    pattern of period 1/2/3/7, random bytes, synthetic text}; every pattern
    continues across the boundary."""
    from lz4 import _synth
    top = max(PREFIX_LENGTHS) + max(BLOCK_LENGTHS)
    rnd = np.random.default_rng(20261020).integers(0, 256, size=top, dtype=np.uint8).tobytes()
    sources = {"zeros": bytes(top), "random": rnd,
               "text": _synth.word_text(np.random.default_rng(6), top).tobytes()}
    for period in (1, 2, 3, 7):
        sources[f"period{period}"] = (bytes(range(0x41, 0x41 + period)) * (top // period + 1))[:top]
    out = []
    for P in PREFIX_LENGTHS:
        for n in BLOCK_LENGTHS:
            for name, s in sources.items():
                out.append((f"{name}-P{P}-n{n}", s[:P], s[P:P + n]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_cases() -> dict:
    """name -> (prefix, block): the edge cases of the prefix parse."""
    rng = np.random.default_rng(65536)

    def rnd(n):
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()

    window = rnd(65536)
    p, q = rnd(100), rnd(100)
    return {
        "dist65535": (window, window[1:1001] + rnd(3000)),      # a match at distance 65535: within reach
        "dist65536": (window, window[0:1000] + rnd(3000)),      # at distance 65536: not
        "back_stop": (p + q + rnd(500) + p, q + rnd(400)),      # equal bytes before both: the match starts at the block
        "run": (b"\x5a" * 300, b"\x5a" * 1000),                 # a run across the boundary
        "short": (window[:5000], window[:12]),                  # below 13 bytes: literals whatever the prefix holds
    }


def linked_frame_parts(data: bytes, level: int, linked: bool, block: int = FRAME_BLOCK) -> list:
    """The model's payload of every block of ``data`` cut into frame blocks
    (linked: each with the up to 64 KiB of input before it as its prefix):
    the compressed block where it fits in block length - 1 bytes, else the raw
    bytes (lz4frame.c:833-842)."""
    buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
    parts = []
    for start in range(0, len(data), block):
        n = min(block, len(data) - start)
        P = min(start, PREFIX_MAX) if linked else 0
        comp = model_compress_at(buf, start, n, P, level, cap=n - 1)
        parts.append(comp if comp is not None else bytes(data[start:start + n]))
    return parts

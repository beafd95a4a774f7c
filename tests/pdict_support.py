"""Shared pieces of tests/test_pdict_args.py and tests/test_gpu_pdict.py: the
inputs of the parallel parse with a shared dictionary
(lz4m_pcompress_dict_batch) and the device round trips the GPU tests use."""
import functools

import numpy as np

BLOCK_LENGTHS = (0, 1, 4, 5, 11, 12, 13, 63, 64, 65, 127, 128, 4096, 65535, 65536)
DICT_LENGTHS = (0, 1, 3, 4, 7, 8, 63, 64, 65, 65535, 65536, 65537, 100_000)
WINDOW = 65536
GUARD = 32          # bytes after every output slot that must stay untouched
GUARD_BYTE = 0xA5

SIZE_KINDS = ("text", "source", "markup", "records", "silesia")
# sum of the oracle's sizes of the 32 blocks of size_case(kind): without a
# dictionary (LZ4_compress_default) and with it (lz4.block.compress(dict=))
ORACLE_TOTALS = {"text": (94936, 74045), "source": (89014, 57771), "markup": (31071, 25489),
                 "records": (88826, 88273), "silesia": (91752, 93124)}


def compress_bound(n: int) -> int:
    return n + n // 255 + 16


@functools.lru_cache(maxsize=None)
def source(kind: str, n: int, seed: int = 5) -> bytes:
    """n bytes of one lz4._synth kind."""
    from lz4 import _synth
    return _synth.KINDS[kind](np.random.default_rng(seed), n).tobytes()


@functools.lru_cache(maxsize=None)
def size_case(kind: str):
    """(D, blocks): the first 192 KiB of six 64 KiB lz4._synth blocks at seed
    31 -- 64 KiB of dictionary, then 32 blocks of 4 KiB."""
    from lz4 import _synth
    buf = _synth.blocks(6, kind, seed=31).reshape(-1)[:3 * WINDOW].tobytes()
    return buf[:WINDOW], [buf[WINDOW + 4096 * i: WINDOW + 4096 * (i + 1)] for i in range(32)]


def grid_case(kind: str, dict_len: int):
    """(D, blocks of BLOCK_LENGTHS) cut one after the other from one buffer of
    ``kind``: the blocks continue the dictionary's data."""
    buf = source(kind, max(DICT_LENGTHS) + sum(BLOCK_LENGTHS))
    blocks, pos = [], dict_len
    for n in BLOCK_LENGTHS:
        blocks.append(buf[pos:pos + n])
        pos += n
    return buf[:dict_len], blocks


@functools.lru_cache(maxsize=None)
def edge_cases() -> dict:
    """name -> (D, block): the boundary and window edges of the parse."""
    rng = np.random.default_rng(65536)

    def rnd(n):
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()

    text = source("text", WINDOW, seed=9)
    head = rnd(64)
    far = head + bytes(WINDOW - 64)             # 64 random bytes at the far end of the window
    abc = b"abc" * 4000
    cases = {}
    for k in (5, 20, 64, 1000, 30000):          # the dictionary's last k bytes, then its first k
        cases[f"tail_head_{k}"] = (text, text[-k:] + text[:k])
    cases["abc_across"] = (abc[:1000], abc[1000:7000])                 # a period of 3 from the dictionary on
    cases["byte_across"] = (b"\x5a" * 300, b"\x5a" * 1000)             # a run of one byte value
    # the only candidates are in the dictionary's last 20 bytes: their matches straddle the boundary
    cases["abc_last_20"] = (rnd(500) + abc[:20], abc[20:620] + rnd(100))
    cases["byte_last_7"] = (rnd(900) + b"\x11" * 7, b"\x11" * 500 + rnd(50))
    cases["dist65535"] = (far, head[1:] + rnd(3000))                   # the only source: at distance 65535
    cases["dist65536"] = (far, head + rnd(3000))                       # at distance 65536: out of reach
    cases["whole_dict"] = (text, text)                                 # every byte's twin is 65536 back
    return cases


# ------------------------------------------------------------- device side
def device_batch(blocks, dev):
    """(src uint8, src_off int64, src_len int32) device tensors of the blocks
    laid back to back."""
    import torch
    lens = np.array([len(b) for b in blocks], dtype=np.int64)
    offs = np.zeros(len(blocks), dtype=np.int64)
    np.cumsum(lens[:-1], out=offs[1:])
    flat = np.frombuffer(b"".join(blocks) + b"\0", dtype=np.uint8).copy()
    return (torch.from_numpy(flat).to(dev), torch.from_numpy(offs).to(dev),
            torch.from_numpy(lens.astype(np.int32)).to(dev))


def device_dict(D, dev):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(D), dtype=np.uint8).copy()).to(dev)


def compress(blocks, dict_buf, dev, caps=None, **kw):
    """compress_batch(table=PARSE_PARALLEL, dict_buf=) on ``blocks``; every
    output slot (``caps``: default LZ4_compressBound) is followed by GUARD
    bytes of GUARD_BYTE, which are checked.  Returns (outputs, out_len): the
    compressed bytes (None where out_len is 0) and the lengths."""
    import torch
    import lz4.block
    from lz4 import _native as N
    src, off, ln = device_batch(blocks, dev)
    caps = [compress_bound(len(b)) for b in blocks] if caps is None else list(caps)
    d_off = np.zeros(len(blocks), dtype=np.int64)
    np.cumsum(np.array(caps[:-1], dtype=np.int64) + GUARD, out=d_off[1:])
    dst = torch.full((int(sum(caps)) + GUARD * len(blocks) + 1,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    if dict_buf is not None:
        kw["dict_buf"] = dict_buf
    _, _, out_len = lz4.block.compress_batch(src, off, ln, table=N.PARSE_PARALLEL, dst=dst,
                                             dst_off=torch.from_numpy(d_off).to(dev),
                                             dst_cap=torch.tensor(caps, dtype=torch.int32, device=dev), **kw)
    out_len = out_len.cpu().tolist()
    host = dst.cpu().numpy()
    outs = []
    for i, L in enumerate(out_len):
        o = int(d_off[i])
        assert 0 <= L <= caps[i], (i, L, caps[i])
        assert (host[o + caps[i]: o + caps[i] + GUARD] == GUARD_BYTE).all(), f"block {i}: bytes written past its slot"
        if L == 0:   # a block that does not fit writes nothing at or past its capacity
            outs.append(None)
        else:
            outs.append(host[o:o + L].tobytes())
    return outs, out_len


def check_decodes(orc, blocks, comps, D):
    """Every block decodes to its input with D as the dictionary: by the CPU
    oracle (LZ4_decompress_safe_usingDict restated) and by the device."""
    import lz4.block
    for i, (b, c) in enumerate(zip(blocks, comps)):
        assert c is not None, f"block {i} ({len(b)} bytes) was not compressed"
        assert len(c) <= compress_bound(len(b)), (i, len(c), len(b))
        r, back = orc.decompress(c, len(b), dict_=D)
        assert r == len(b) and back == b, f"block {i} ({len(b)} bytes, dictionary {len(D)}): oracle status {r}"
    back = lz4.block.decompress_many(comps, uncompressed_size=[len(b) for b in blocks], dict=D)
    assert back == list(blocks)

"""GPU parity of the HIP block codec against the CPU oracle (bit-exact).

Everything here calls the HIP kernels through the C-ABI library
(``lz4._native`` -> ``_lz4m.so``); the oracle (oracle/lz4_oracle.c, pinned to
the reference by tests/test_oracle.py and tests/golden) is only the checker.
"""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lz4 import _native as N
from lz4 import _synth

from layout_support import malformed_cases, _literal_block, _long_sequence_blocks, _offset0_block


def _pack(blocks):
    offs, lens, total = [], [], 0
    for b in blocks:
        offs.append(total)
        lens.append(len(b))
        total += len(b)
    return b"".join(blocks), offs, lens


# every decoder (include/lz4m.h lz4m_decompress_batch_sel) must give the
# reference's bytes and statuses; "auto" is the size-based default
DECODERS = ["auto", "rows", "hist"]


def gpu_decompress(blocks, caps, dev, decoder="auto"):
    packed, offs, lens = _pack(blocks)
    d_src = N.to_device(packed, dev)
    d_off, acc = [], 0
    for c in caps:
        d_off.append(acc)
        acc += max(c, 0)
    d_dst = torch.zeros(max(acc, 1), dtype=torch.uint8, device=dev)
    st = torch.empty(len(blocks), dtype=torch.int32, device=dev)
    N.launch_decompress(d_src, torch.tensor(offs, dtype=torch.int64, device=dev),
                        torch.tensor(lens, dtype=torch.int32, device=dev), d_dst,
                        torch.tensor(d_off, dtype=torch.int64, device=dev),
                        torch.tensor(caps, dtype=torch.int32, device=dev), st, len(blocks), decoder=decoder)
    host = d_dst.cpu().numpy()
    out = []
    for i, s in enumerate(st.cpu().tolist()):
        out.append((s, host[d_off[i]:d_off[i] + s].tobytes() if s > 0 else b""))
    return out


def gpu_compress(blocks, table, dev, accel=1, caps=None, max_len=None):
    packed, offs, lens = _pack(blocks)
    caps = caps or [N.compress_bound(L) for L in lens]
    d_src = N.to_device(packed, dev)
    d_off, acc = [], 0
    for c in caps:
        d_off.append(acc)
        acc += max(c, 1)
    d_dst = torch.zeros(max(acc, 1), dtype=torch.uint8, device=dev)
    ol = torch.empty(len(blocks), dtype=torch.int32, device=dev)
    N.launch_compress(d_src, torch.tensor(offs, dtype=torch.int64, device=dev),
                      torch.tensor(lens, dtype=torch.int32, device=dev), d_dst,
                      torch.tensor(d_off, dtype=torch.int64, device=dev),
                      torch.tensor(caps, dtype=torch.int32, device=dev), ol, len(blocks), table, accel,
                      max_len=max_len)
    host = d_dst.cpu().numpy()
    return [host[d_off[i]:d_off[i] + L].tobytes() if L > 0 else None for i, L in enumerate(ol.cpu().tolist())]


@pytest.fixture(scope="module")
def corpus():
    blocks = [b.tobytes() for b in _synth.blocks(96, "silesia", seed=11)]
    rng = random.Random(5)
    # ragged sizes, including every edge the format defines (0..13, 64K limit)
    sizes = [0, 1, 4, 5, 11, 12, 13, 14, 15, 16, 17, 31, 32, 63, 64, 65, 100, 255, 256, 1000, 4095, 4096,
             65535, 65536]
    ragged = []
    for s in sizes:
        b = blocks[rng.randrange(len(blocks))]
        ragged.append(b[:s])
    return blocks, ragged


@pytest.mark.parametrize("decoder", DECODERS)
def test_decompress_matches_oracle(gpu, oracle, corpus, decoder):
    blocks, ragged = corpus
    src = blocks + ragged + [bytes(65536), bytes([7]) * 65536, b"ab" * 32768]
    comp = [oracle.compress(b) for b in src]
    res = gpu_decompress(comp, [len(b) for b in src], gpu, decoder)
    for i, (s, out) in enumerate(res):
        assert s == len(src[i]), (i, s, len(src[i]))
        assert out == src[i], i


@pytest.mark.parametrize("variant", [N.TABLE_U16_HASH4, N.TABLE_U32_HASH5])
def test_compress_bit_exact(gpu, oracle, corpus, variant):
    blocks, ragged = corpus
    src = blocks[:48] + ragged + [bytes(65536), bytes([7]) * 65536, b"ab" * 32768]
    got = gpu_compress(src, variant, gpu)
    for i, b in enumerate(src):
        want = oracle.compress(b, variant)
        assert got[i] == want, (i, len(b), None if got[i] is None else len(got[i]), len(want))


def test_compress_acceleration(gpu, oracle, corpus):
    blocks, _ = corpus
    for accel in (2, 7, 100, 70000):
        got = gpu_compress(blocks[:16], N.TABLE_U32_HASH5, gpu, accel=accel)
        for i, b in enumerate(blocks[:16]):
            assert got[i] == oracle.compress(b, N.TABLE_U32_HASH5, accel=accel), (accel, i)


def test_compress_limited_output(gpu, oracle, corpus):
    blocks, _ = corpus
    src = blocks[:24]
    caps = [len(b) - 1 for b in src]   # frame block capacity (lz4frame.c:835)
    got = gpu_compress(src, N.TABLE_U16_HASH4, gpu, caps=caps)
    for i, b in enumerate(src):
        want = oracle.compress(b, N.TABLE_U16_HASH4, cap=caps[i])
        assert got[i] == want, i


def test_compress_large_block_u32(gpu, oracle, corpus):
    blocks, _ = corpus
    big = b"".join(blocks[:20])   # 1.25 MiB, byU32 with distance check
    got = gpu_compress([big], N.TABLE_U32_HASH5, gpu)[0]
    assert got == oracle.compress(big, N.TABLE_U32_HASH5)


@pytest.mark.parametrize("decoder", DECODERS)
def test_decompress_malformed_matches_oracle(gpu, oracle, corpus, decoder):
    blocks, _ = corpus
    cases, caps = malformed_cases(oracle, blocks)
    res = gpu_decompress(cases, caps, gpu, decoder)
    for i, (s, out) in enumerate(res):
        want = oracle.decompress(cases[i], caps[i])
        assert s == want[0], (i, s, want[0], caps[i])
        if s >= 0:
            assert out == want[1], i


@pytest.mark.parametrize("decoder", DECODERS)
def test_decompress_random_garbage(gpu, oracle, decoder):
    rng = np.random.default_rng(3)
    cases = [rng.integers(0, 256, size=int(rng.integers(1, 300)), dtype=np.uint8).tobytes() for _ in range(2000)]
    caps = [int(rng.integers(0, 5000)) for _ in cases]
    res = gpu_decompress(cases, caps, gpu, decoder)
    for i, (s, out) in enumerate(res):
        want = oracle.decompress(cases[i], caps[i])
        assert s == want[0], (i, s, want[0])
        if s >= 0:
            assert out == want[1]


def test_decompress_dict(gpu, oracle, corpus):
    blocks, _ = corpus
    from lz4.block import decompress_many
    d = blocks[0][:30000]
    # build blocks that reference a dictionary: compress dict+data and strip
    # the dictionary part is not possible with the plain compressor; instead
    # check that dict-mode decode of ordinary blocks and of crafted blocks
    # with offsets reaching into the dictionary matches the oracle.
    crafted = []
    for k in range(64):
        lit = bytes([65 + k % 26]) * 3
        off = 30 + k * 100
        ml = 20 + k
        seq = bytes([(3 << 4) | 15]) + lit + off.to_bytes(2, "little") + bytes([ml - 19])
        tail = b"END__"
        crafted.append(seq + bytes([len(tail) << 4]) + tail)
    caps = [3 + 20 + k + 5 + 10 for k in range(64)]
    res = decompress_many(crafted, uncompressed_size=caps, dict=d, raise_errors=False)
    for i, c in enumerate(crafted):
        s, want = oracle.decompress(c, caps[i], dict_=d)
        if s < 0:
            assert not isinstance(res[i], (bytes, bytearray))
            assert str(-s) in str(res[i])
        else:
            assert res[i] == want, i


def test_xxh32_batch(gpu, oracle, corpus):
    blocks, ragged = corpus
    # lengths around the lane loop's 8-stripe prefetch groups (128 / 256 B)
    edge = [blocks[0][:k] for k in (0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 271, 272, 383, 384, 385,
                                   511, 512, 4095, 34567)]
    items = blocks[:32] + ragged + edge
    packed, offs, lens = _pack(items)
    d = N.to_device(packed, gpu)
    out = torch.empty(len(items), dtype=torch.int32, device=gpu)
    for seed in (0, 1, 0x9E3779B1):
        N.launch_xxh32_batch(d, torch.tensor(offs, dtype=torch.int64, device=gpu),
                             torch.tensor(lens, dtype=torch.int64, device=gpu), seed, out, len(items))
        got = [v & 0xFFFFFFFF for v in out.cpu().tolist()]
        assert got == [oracle.xxh32(b, seed) for b in items]


def test_lds_lane_order_selftest(gpu):
    """The exact and parallel-parse compressors insert a search step's
    positions with one LDS exchange per lane and rely on the lanes of one
    instruction that hit the same entry being applied in lane order (the
    serial insert order of lz4.c:1016-1075).  The library runs this check
    once per process before compressing; here it must report no violation."""
    assert N.lib().lz4m_selftest_lds_order() == 0


def test_xxh32_batch_page(gpu, oracle):
    """The quad-per-item batch kernel on a config-5-like page: 4 101 items
    (not a multiple of the 16 items a wave takes) of 0..70 000 bytes at any
    alignment, overlapping slices of one buffer, wave-mates of very different
    lengths (items with no full stripe next to 64 KiB ones), against the
    oracle's XXH32 (xxhash.c:392-416)."""
    rng = np.random.default_rng(5)
    buf = rng.integers(0, 256, 8 << 20, dtype=np.uint8)
    n = 4101
    lens = rng.integers(0, 70000, n)
    lens[rng.integers(0, n, 300)] = rng.integers(0, 16, 300)   # tails only
    lens[:16] = [0, 1, 15, 16, 17, 31, 32, 33, 65536, 3, 70000, 0, 48, 49, 1000, 5]
    offs = rng.integers(0, len(buf) - 70000, n)
    d = torch.from_numpy(buf).to(gpu)
    out = torch.empty(n, dtype=torch.int32, device=gpu)
    N.launch_xxh32_batch(d, torch.tensor(offs, dtype=torch.int64, device=gpu),
                         torch.tensor(lens, dtype=torch.int64, device=gpu), 0x1234567, out, n)
    got = [v & 0xFFFFFFFF for v in out.cpu().tolist()]
    want = [oracle.xxh32(buf[o:o + k].tobytes(), 0x1234567) for o, k in zip(offs, lens)]
    assert got == want


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 63, 64, 511, 512, 513, 1023, 1024, 1025, 4096 + 7,
                               3 * 65536 + 5, (1 << 20) + 77])
@pytest.mark.parametrize("shift", [0, 1, 3, 4])
def test_xxh32_long(gpu, oracle, corpus, n, shift):
    """Content-checksum kernel (scalar-loaded path for dword-aligned sources,
    vector path otherwise) against the oracle's XXH32, several seeds."""
    blocks, _ = corpus
    data = (b"".join(blocks) * 2)[:n]
    d = N.to_device(b"\x00" * shift + data, gpu, pad=1)[shift:]
    out = torch.empty(1, dtype=torch.int32, device=gpu)
    for seed in (0, 0x9E3779B1):
        N.launch_xxh32_long(d, n, seed, out)
        assert out.item() & 0xFFFFFFFF == oracle.xxh32(data, seed)


@pytest.mark.parametrize("wait", ["event", "stream"])
def test_xxh32_of_device(gpu, wait):
    """The host-core hash of device bytes (xxh32_of_device, one span of
    xxh32_of_device_spans) against the host hash of the same bytes, at the
    sizes where the two-buffer alternation and the tail can go wrong around
    a 4 096-byte chunk; the bytes are produced on a side stream that the hash
    waits for through an event or through the stream itself."""
    chunk = 4096
    buf = np.random.default_rng(11).integers(0, 256, 2 * chunk + 3, dtype=np.uint8)
    base = torch.from_numpy(buf).to(gpu)
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        t = base.clone()
        ev = torch.cuda.Event()
        ev.record(s)
    kw = {"wait_event": ev} if wait == "event" else {"wait_stream": s}
    for n in (0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 3):
        for seed in (0, 0x9E3779B1):
            assert N.xxh32_of_device(t, n, seed, chunk=chunk, **kw) == N.xxh32_host(buf[:n].tobytes(), seed), (n, seed)
    s.synchronize()


_STAGE_BIG, _STAGE_CHUNK = 1 << 16, 1 << 18


@pytest.mark.parametrize("n", [_STAGE_BIG, _STAGE_CHUNK - 1, _STAGE_CHUNK, _STAGE_CHUNK + 1, 2 * _STAGE_CHUNK,
                               3 * _STAGE_CHUNK + 5])
def test_staged_host_device_copies(gpu, oracle, monkeypatch, n):
    """The chunked large paths of to_device and to_host_bytes (two pinned
    chunks), with the thresholds lowered so that a few hundred KiB cover the
    smallest large size, one chunk less and more than a byte, ends exactly on
    a chunk edge, and a third chunk that reuses buffer 0: the bytes, the zero
    pad, the result type and the streamed XXH32 (against the oracle's)."""
    monkeypatch.setattr(N, "_BIG", _STAGE_BIG)
    monkeypatch.setattr(N, "_CHUNK", _STAGE_CHUNK)
    data = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    want = {seed: oracle.xxh32(data, seed) for seed in (0, 0x9E3779B1)}
    for pad in (0, 16):
        d = N.to_device(data, gpu, pad=pad)
        assert d.dtype == torch.uint8 and d.numel() == n + pad
        assert not bool(d[n:].any()), pad
        for as_bytearray in (False, True):
            for seed in (None, 0, 0x9E3779B1):
                r = N.to_host_bytes(d, n, as_bytearray, hash_seed=seed)
                out, digest = r if seed is not None else (r, None)
                assert type(out) is (bytearray if as_bytearray else bytes), (pad, as_bytearray, seed)
                assert out == data, (pad, as_bytearray, seed)
                if seed is not None:
                    assert digest == want[seed], (pad, as_bytearray, seed)


def test_scan_and_gather(gpu):
    rng = np.random.default_rng(0)
    for n in (1, 5, 2047, 2048, 2049, 100000):
        lens = rng.integers(0, 300, size=n).astype(np.int32)
        t = torch.tensor(lens, device=gpu)
        offs = N.exclusive_scan(t, add=3, base=11).cpu().numpy()
        want = np.concatenate([[0], np.cumsum(lens.astype(np.int64) + 3)]) + 11
        assert (offs == want).all(), n


# ---------------------------------------------------------------- parallel parse
def _decodes(oracle, comp, plain):
    st, out = oracle.decompress(comp, len(plain))
    return st == len(plain) and out == plain


def test_parallel_parse_valid(gpu, oracle, corpus):
    """Every block the parallel-parse compressor emits is a valid LZ4 block
    that the reference decoder (oracle, pinned to lz4libs) decodes exactly."""
    blocks, ragged = corpus
    src = blocks + ragged + [bytes(65536), bytes([7]) * 65536, b"ab" * 32768, b"abc" * 21845,
                             bytes(range(256)) * 256]
    for variant in (N.PARSE_PARALLEL, N.PARSE_PARALLEL_HQ):
        got = gpu_compress(src, variant, gpu)
        for i, b in enumerate(src):
            assert got[i] is not None and len(got[i]) <= N.compress_bound(len(b)), (variant, i)
            assert _decodes(oracle, got[i], b), (variant, i, len(b))


@pytest.mark.parametrize("kind", ["text", "source", "records", "markup", "runs", "random", "silesia"])
@pytest.mark.parametrize("variant,tol", [(N.PARSE_PARALLEL, 1.05), (N.PARSE_PARALLEL_HQ, 1.02)])
def test_parallel_parse_ratio(gpu, oracle, kind, variant, tol):
    """Size within 5 % of LZ4_compress_default (BASELINE config 3), per kind,
    for the 12-bit table; within 2 % for the 13-bit (HQ) table."""
    src = [b.tobytes() for b in _synth.blocks(24, kind, seed=31)]
    got = gpu_compress(src, variant, gpu)
    ours = sum(len(g) for g in got)
    ref = sum(len(oracle.compress(b)) for b in src)
    assert ours <= tol * ref, (kind, ours, ref)
    for g, b in zip(got, src):
        assert _decodes(oracle, g, b)


@pytest.mark.parametrize("seg", [True, False])
@pytest.mark.parametrize("kind", ["text", "markup", "runs", "random", "silesia"])
def test_parallel_parse_large_blocks(gpu, oracle, kind, seg):
    """PARSE_PARALLEL_LARGE (blocks > 64 KiB: frame blocks of 256 KiB - 4 MiB)
    on 4 MiB, odd and just-over-64-KiB blocks, plus periodic data whose
    repeats sit at offsets 65535 / 65536 / 65537 (the window edge: a match at
    distance 65536 is not encodable, lz4.c:1064).  Every block decodes
    exactly with the reference decoder and stays within 5 % of
    LZ4_compress_default's size.  seg: the segmented parse
    (lz4m_pcompress_large_batch, what lz4.frame uses) or one wavefront per
    block."""
    raw = _synth.blocks(2 * 64 + 8, kind, seed=41).tobytes()
    src = [raw[:4 << 20], raw[(4 << 20):(4 << 20) + 300_001], raw[-65537:]]
    rng = np.random.default_rng(5)
    for period in (65535, 65536, 65537):
        unit = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
        src.append((unit * 4)[:3 * period + 1000])
    got = gpu_compress(src, N.PARSE_PARALLEL_LARGE, gpu, max_len=max(map(len, src)) if seg else None)
    for i, b in enumerate(src):
        assert got[i] is not None and len(got[i]) <= N.compress_bound(len(b)), i
        assert _decodes(oracle, got[i], b), (i, len(b))
    ours = sum(len(g) for g in got[:3])
    ref = sum(len(oracle.compress(b)) for b in src[:3])
    assert ours <= 1.05 * ref, (kind, ours, ref)


def test_parallel_parse_segment_joins(gpu, oracle):
    """The segmented large-block parse (lz4m_pcompress_large_batch): segment
    edges at every size class -- one segment, a last segment of 1, 2, 3 and
    13 bytes, segments longer than 256 KiB (blocks over 4 MiB), empty blocks
    -- and literals carried across segments without a match (incompressible
    segments before compressible ones: the first sequence after them takes
    a literal run of ~700 KiB).  Every block decodes exactly with the
    reference decoder; a block whose joined size exceeds its capacity
    reports 0 (None)."""
    rng = np.random.default_rng(9)
    text = _synth.blocks(160, "text", seed=3).tobytes()
    seg = 256 << 10
    src = [b"", b"abcd" * 3, text[:seg], text[:seg + 1], text[:seg + 2], text[:seg + 3], text[:2 * seg + 13],
           text[:(4 << 20) + 4097], text[:5 * seg + 17],
           rng.integers(0, 256, 700 << 10, dtype=np.uint8).tobytes() + text[:500 << 10],
           rng.integers(0, 256, seg, dtype=np.uint8).tobytes() + b"z" * 5 + rng.integers(0, 256, seg, dtype=np.uint8).tobytes(),
           text[:seg] + rng.integers(0, 256, 3 * seg, dtype=np.uint8).tobytes()]
    got = gpu_compress(src, N.PARSE_PARALLEL_LARGE, gpu, max_len=max(map(len, src)))
    for i, b in enumerate(src):
        assert got[i] is not None and len(got[i]) <= N.compress_bound(len(b)), i
        assert _decodes(oracle, got[i], b), (i, len(b))
    # limited output: an incompressible block does not fit size - 1; a compressible one does
    noise = rng.integers(0, 256, 3 * seg, dtype=np.uint8).tobytes()
    lim = [noise, text[:3 * seg]]
    got = gpu_compress(lim, N.PARSE_PARALLEL_LARGE, gpu, caps=[len(b) - 1 for b in lim], max_len=3 * seg)
    assert got[0] is None
    assert got[1] is not None and _decodes(oracle, got[1], lim[1])


def test_parallel_parse_limited_output(gpu, oracle, corpus):
    blocks, _ = corpus
    noise = np.random.default_rng(3).integers(0, 256, 65536, dtype=np.uint8).tobytes()
    src = blocks[:24] + [bytes(range(256)) * 256, noise]
    caps = [len(b) - 1 for b in src]
    got = gpu_compress(src, N.PARSE_PARALLEL, gpu, caps=caps)
    for i, b in enumerate(src):
        if got[i] is not None:
            assert len(got[i]) <= caps[i] and _decodes(oracle, got[i], b), i
    assert got[-1] is None   # incompressible block does not fit size - 1


def test_parallel_parse_decoded_by_gpu(gpu, corpus):
    blocks, ragged = corpus
    src = blocks[:32] + ragged
    got = gpu_compress(src, N.PARSE_PARALLEL, gpu)
    res = gpu_decompress(got, [len(b) for b in src], gpu)
    for i, (s, out) in enumerate(res):
        assert s == len(src[i]) and out == src[i], i


@pytest.mark.parametrize("decoder", DECODERS)
@pytest.mark.parametrize("kind", ["text", "source", "markup", "records", "runs", "random"])
@pytest.mark.parametrize("block", [65536, 4 << 20, 300_001])
def test_decompress_kinds_and_sizes(gpu, oracle, kind, block, decoder):
    """The hot decoder on every corpus kind at 64 KiB, 4 MiB and an odd
    block size: long matches (markup: ml > 16 on 70 % of sequences), offsets
    around the LDS ring's reach, runs and incompressible blocks, positions
    beyond 64 KiB.  Blocks come from the oracle (LZ4_compress_default);
    output and status must equal the original bytes and size."""
    n = 48 if block == 65536 else 3
    raw = _synth.blocks(n * block // 65536 + 1, kind, seed=31).tobytes()
    blocks = [raw[i * block:(i + 1) * block] for i in range(n)]
    comp = [oracle.compress(b) for b in blocks]
    got = gpu_decompress(comp, [block] * n, gpu, decoder)
    for (st, out), b in zip(got, blocks):
        assert st == len(b) and out == b


@pytest.mark.parametrize("decoder", DECODERS)
def test_decompress_whole_literal_blocks(gpu, oracle, decoder):
    """Incompressible blocks -- one literal running exactly to the block's end,
    which the row decoder's parse kernel decodes itself (whole_literal_block,
    lz4m_rows.hip; the reference's last-literals branch, lz4.c:2172-2229) --
    and every near miss, which must keep the reference's status: one byte
    short or long, a capacity one below, a match after the literal, a run
    longer than the 1 KiB the check reads, a literal shorter than the parse's
    length-run cap.  Statuses and bytes equal the oracle's."""
    rng = np.random.default_rng(17)
    cases, caps = [], []
    for L in [15, 300, 4094, 4095, 4096, 4110, 4111, 5000, 65535, 65536, 65537, 100_000, 260_000, 270_000]:
        p = rng.integers(0, 256, size=L, dtype=np.uint8).tobytes()
        b = _literal_block(p)
        for cap in (L, L - 1, L + 100, 64):
            cases.append(b)
            caps.append(cap)
        cases += [b[:-1], b + b"x", _literal_block(p, tok=0xFF), _literal_block(p, tail=b"\x05\x00" + b"\x50abcde"),
                  _literal_block(p, tok=0xF4, tail=b"\x05\x00" + b"\x50abcde")]
        caps += [L, L + 1, L, L + 13, L + 13]
    # a length run that never ends inside the block, and one ending on the
    # read_variable_length limit (ilimit = iend - 15)
    cases += [b"\xf0" + b"\xff" * 5000, b"\xf0" + b"\xff" * 20 + b"\x01" + b"\x00" * 13]
    caps += [1 << 20, 1 << 20]
    # a batch past the row decoder's switch-over for "auto": every 16th block
    # one of the cases above (up to 64 KiB + 1), the rest 2 KiB pieces of the corpus
    small = [i for i in range(len(cases)) if len(cases[i]) < 70_000]
    raw = _synth.blocks(16, "silesia", seed=3).tobytes()
    pool = [oracle.compress(raw[2048 * i:2048 * (i + 1)]) for i in range(64)]
    while len(cases) < 33_000:
        i = len(cases)
        j = small[(i // 16) % len(small)]
        cases.append(cases[j] if i % 16 == 0 else pool[i % 64])
        caps.append(caps[j] if i % 16 == 0 else 2048)
    res = gpu_decompress(cases, caps, gpu, decoder)
    memo = {}
    for i, (s, out) in enumerate(res):
        key = (cases[i], caps[i])
        want = memo.get(key)
        if want is None:
            want = memo[key] = oracle.decompress(cases[i], caps[i])
        assert s == want[0], (i, s, want[0], caps[i])
        if s >= 0:
            assert out == want[1], i


@pytest.mark.parametrize("decoder", DECODERS)
def test_decompress_long_sequences(gpu, oracle, decoder):
    """Sequences the row decoder takes one at a time (rows_exec_kernel's
    one-sequence path: the parsed lane-0 values, or a byte-by-byte re-parse of
    an escaped sequence; far matches in whole-offset steps) and the
    whole-literal path: bytes and statuses equal the oracle's at the exact
    capacity and one below."""
    blocks = _long_sequence_blocks(24, 41)
    comp = [oracle.compress(b) for b in blocks]
    cases = comp + comp
    caps = [65536] * len(comp) + [65535] * len(comp)
    res = gpu_decompress(cases, caps, gpu, decoder)
    for i, (s, out) in enumerate(res):
        want = oracle.decompress(cases[i], caps[i])
        assert s == want[0], (i, s, want[0])
        if s >= 0:
            assert out == want[1], i


@pytest.mark.parametrize("shift", [1, 13, 63])
def test_decompress_unaligned_input_base(gpu, oracle, corpus, shift):
    """The rows parse reads each block through 64-byte windows at absolute
    line boundaries, starting up to 63 bytes before the block -- but never
    before the caller's buffer: an input buffer `shift` bytes past a line,
    first blocks at offsets 0..62 (rows_parse_kernel's `sh`)."""
    blocks, ragged = corpus
    src = [b[:17 + 7 * i] for i, b in enumerate(blocks[:9])] + blocks[:24] + ragged
    comp = [oracle.compress(b) for b in src]
    packed, offs, lens = _pack(comp)
    base = torch.zeros(len(packed) + 64 + shift, dtype=torch.uint8, device=gpu)
    view = base[shift:shift + len(packed)]
    view.copy_(torch.frombuffer(bytearray(packed), dtype=torch.uint8).to(gpu))
    caps = [max(len(b), 1) for b in src]
    d_off = np.concatenate([[0], np.cumsum(caps)[:-1]]).tolist()
    dst = torch.zeros(sum(caps), dtype=torch.uint8, device=gpu)
    st = torch.empty(len(src), dtype=torch.int32, device=gpu)
    N.launch_decompress(view, torch.tensor(offs, dtype=torch.int64, device=gpu),
                        torch.tensor(lens, dtype=torch.int32, device=gpu), dst,
                        torch.tensor(d_off, dtype=torch.int64, device=gpu),
                        torch.tensor(caps, dtype=torch.int32, device=gpu), st, len(src), decoder="rows")
    host = dst.cpu().numpy()
    for i, s in enumerate(st.cpu().tolist()):
        want = oracle.decompress(comp[i], caps[i])
        assert s == want[0], (i, s, want[0])
        if s > 0:
            assert host[d_off[i]:d_off[i] + s].tobytes() == want[1], i


@pytest.mark.parametrize("decoder", ["auto", "hist"])
def test_decompress_large_batch_edges(gpu, oracle, corpus, decoder):
    """A batch above the small-batch switch-over (32 768 blocks), so the
    default dispatch runs the large-batch decoder, with every edge case of the
    small tests embedded: the golden decode vectors with their capacities,
    3 000 mutated / truncated blocks, random garbage, ragged sizes 0..65536,
    offset-0 blocks and capacities below the size.  Statuses and bytes must
    equal the oracle's (lz4libs/lz4.c:1936-2339)."""
    import json
    import os
    from conftest import GOLDEN
    blocks, ragged = corpus
    cases, caps = [], []
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    arr = np.load(os.path.join(GOLDEN, "golden.npz"), allow_pickle=False)
    for e in man["decompress"]:
        cases.append(arr[e["key"]].tobytes())
        caps.append(e["cap"])
    mc, mcap = malformed_cases(oracle, blocks)
    cases += mc
    caps += mcap
    rng = np.random.default_rng(9)
    for _ in range(1000):
        cases.append(rng.integers(0, 256, size=int(rng.integers(1, 300)), dtype=np.uint8).tobytes())
        caps.append(int(rng.integers(0, 5000)))
    for r in ragged + blocks[:8]:
        c = oracle.compress(r)
        for cap in {len(r), max(0, len(r) - 1), len(r) + 7, max(0, len(r) - 70)}:
            cases.append(c)
            caps.append(cap)
    for k in range(64):
        b = _offset0_block(bytes([65 + k % 26]) * (k % 13), 4 + k % 11)
        cases.append(b)
        caps.append(k % 13 + 4 + k % 11 + 5 + (k % 3) * 40)
    # fill with small valid blocks (pieces of the corpus) past the switch-over
    pool = [oracle.compress(blocks[i % len(blocks)][(i * 97) % 60000:(i * 97) % 60000 + 64 + i % 700])
            for i in range(512)]
    want_len = [64 + i % 700 for i in range(512)]
    i = 0
    while len(cases) < 100_000:
        cases.append(pool[i % 512])
        caps.append(want_len[i % 512])
        i += 1
    res = gpu_decompress(cases, caps, gpu, decoder)
    memo = {}
    for i, (s, out) in enumerate(res):
        key = (cases[i], caps[i])
        want = memo.get(key)
        if want is None:
            want = memo[key] = oracle.decompress(cases[i], caps[i])
        assert s == want[0], (i, s, want[0], caps[i])
        if s >= 0:
            assert out == want[1], i


def test_host_single_block_functions(gpu, oracle, corpus):
    """lz4m_decompress_safe / lz4m_compress_default / lz4m_compress_block_api /
    lz4m_xxh32: host pointers, lz4.h contracts, equal to the oracle."""
    import ctypes as C
    lib = N.lib()
    blocks, ragged = corpus
    for b in blocks[:6] + ragged:
        cap = N.compress_bound(len(b))
        out = C.create_string_buffer(max(cap, 1))
        n = lib.lz4m_compress_default(b, out, len(b), cap)
        assert out.raw[:n] == oracle.compress(b), len(b)
        n2 = lib.lz4m_compress_block_api(b, out, len(b), cap, 1)
        assert out.raw[:n2] == oracle.compress(b, variant=1), len(b)
        comp = oracle.compress(b)
        dec = C.create_string_buffer(max(len(b), 1))
        assert lib.lz4m_decompress_safe(comp, dec, len(comp), len(b)) == len(b)
        assert dec.raw[:len(b)] == b
        assert lib.lz4m_xxh32(b, len(b), 7) == oracle.xxh32(b, 7)
    # limited output and a corrupt block: the reference's return values
    b = blocks[0]
    comp = oracle.compress(b)
    out = C.create_string_buffer(16)
    assert lib.lz4m_compress_default(b, out, len(b), 16) == 0
    dec = C.create_string_buffer(len(b))
    bad = bytearray(comp)
    bad[len(bad) // 2] ^= 0xFF
    assert lib.lz4m_decompress_safe(bytes(bad), dec, len(bad), len(b)) == \
        oracle.decompress(bytes(bad), len(b))[0]


def _phrases(n_bytes: int, seed: int) -> bytes:
    """High-ratio data made of 60-250 byte slices of a small vocabulary: LZ4
    matches of ~60-250 bytes, ~90 decoded bytes per sequence."""
    rng = np.random.default_rng(seed)
    vocab = rng.integers(0, 256, size=(64, 400), dtype=np.uint8)
    out, total = [], 0
    while total < n_bytes:
        L = int(rng.integers(60, 251))
        w = vocab[int(rng.integers(0, 64))]
        a = int(rng.integers(0, 400 - L))
        out.append(w[a:a + L].tobytes())
        total += L
    return b"".join(out)[:n_bytes]


@pytest.mark.parametrize("decoder", DECODERS)
@pytest.mark.parametrize("block", [65536, 4 << 20])
def test_decompress_high_ratio(gpu, oracle, decoder, block):
    """Mid-length matches (60-250 B, ~90 B per sequence): rounds of the
    on-chip-history decoders fill their buffers long before 64 sequences, so
    a round cut by buffer space must go on after a rebase, and
    the output must still equal the oracle's."""
    blocks = [_phrases(block, 40 + i) for i in range(3 if block > 65536 else 24)]
    comp = [oracle.compress(b) for b in blocks]
    got = gpu_decompress(comp, [block] * len(blocks), gpu, decoder)
    for (st, out), b in zip(got, blocks):
        assert st == len(b) and out == b


def test_decompress_prefix_matches_oracle(gpu, oracle, corpus):
    """lz4m_decompress_batch_prefix (the linked-frame decoder: each block's
    dictionary ends where its slot starts, in a second buffer laid out like
    the output) against the oracle's
    LZ4_decompress_safe_usingDict (lz4.c:2612-2625), on blocks compressed
    against dictionaries of 0 B .. 64 KiB, mutated / truncated copies and
    capacities around the true size; nothing outside a slot is written."""
    blocks, _ = corpus
    rng = random.Random(77)
    cases = []
    for i in range(700):
        b = blocks[rng.randrange(len(blocks))]
        dl = rng.choice([0, 5, 16, 100, 5000, 30000, 65536])
        n = rng.choice([100, 2000, 20000, 65536 - dl if dl < 65536 else 65536])
        n = max(1, min(n, 65536))
        joined = b + blocks[rng.randrange(len(blocks))]
        start = rng.randrange(0, len(joined) - (dl + n) + 1) if len(joined) >= dl + n else 0
        dic, data = joined[start:start + dl], joined[start + dl:start + dl + n]
        c = bytearray(oracle.compress_dict(data, dic) if dl >= 8 else oracle.compress(data))
        if i % 3 == 1:
            for _ in range(rng.randrange(1, 4)):
                c[rng.randrange(len(c))] = rng.randrange(256)
        if i % 7 == 2:
            c = c[:rng.randrange(len(c) + 1)]
        cap = rng.choice([len(data), len(data), len(data) - 1, len(data) + 77, max(0, len(data) - 9)])
        cases.append((dic, bytes(c), cap, len(data)))
    # two buffers laid out alike: the output [gap][slot_i (cap_i)][64-byte guard] ..., and the
    # dictionaries, dict_i ending where slot_i starts (the output's gaps hold a sentinel)
    out_b, dic_b, doff, dl, caps = bytearray(), bytearray(), [], [], []
    for dic, c, cap, _ in cases:
        out_b += b"\x5A" * len(dic)
        dic_b += dic
        doff.append(len(out_b))
        dl.append(len(dic))
        caps.append(cap)
        out_b += b"\xA5" * (cap + 64)
        dic_b += b"\x00" * (cap + 64)
    packed, offs, lens = _pack([c for _, c, _, _ in cases])
    dev = gpu
    d_src = torch.frombuffer(bytearray(packed), dtype=torch.uint8).to(dev)
    d_out = torch.frombuffer(bytearray(out_b), dtype=torch.uint8).to(dev)
    d_dic = torch.frombuffer(bytearray(dic_b), dtype=torch.uint8).to(dev)
    so = torch.tensor(offs, dtype=torch.int64, device=dev)
    sl = torch.tensor(lens, dtype=torch.int32, device=dev)
    do = torch.tensor(doff, dtype=torch.int64, device=dev)
    dc = torch.tensor(caps, dtype=torch.int32, device=dev)
    dd = torch.tensor(dl, dtype=torch.int32, device=dev)
    st = torch.empty(len(cases), dtype=torch.int32, device=dev)
    N.launch_decompress_prefix(d_src, so, sl, d_out, do, dc, d_dic, dd, st, len(cases))
    torch.cuda.synchronize()
    out, status = bytes(d_out.cpu().numpy()), st.cpu().tolist()
    assert bytes(d_dic.cpu().numpy()) == bytes(dic_b), "the dictionary buffer was written"
    for i, (dic, c, cap, n) in enumerate(cases):
        want_s, want = oracle.decompress(c, cap, dict_=dic if dic else None)
        assert status[i] == want_s, (i, len(dic), cap, status[i], want_s)
        o = doff[i]
        if want_s >= 0:
            assert out[o:o + want_s] == want, i
        assert out[o + cap:o + cap + 64] == b"\xA5" * 64, ("wrote past the slot", i)
        assert out[o - len(dic):o] == b"\x5A" * len(dic), ("wrote before the slot", i)

"""The parallel parse with a shared dictionary on the device
(lz4m_pcompress_dict_batch; compress_batch(dict_buf=), prepare_dict,
compress_many(dict=, table=PARSE_PARALLEL)): DESIGN.md section 3.8."""
import numpy as np
import pytest

import pdict_support as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["text", "random"])
def test_every_block_decodes_with_the_dictionary(gpu, oracle, kind):
    """Block lengths x dictionary lengths (only its last 64 KiB count): every
    output is within LZ4_compressBound and decodes to its input with the
    dictionary, by the CPU oracle and by the device decoder."""
    for dl in P.DICT_LENGTHS:
        D, blocks = P.grid_case(kind, dl)
        comps, _ = P.compress(blocks, P.device_dict(D, gpu), gpu)
        P.check_decodes(oracle, blocks, comps, D)


def test_boundary_and_window_edges(gpu, oracle):
    cases = P.edge_cases()
    sizes = {}
    for name, (D, block) in cases.items():
        comps, out_len = P.compress([block], P.device_dict(D, gpu), gpu)
        P.check_decodes(oracle, [block], comps, D)
        sizes[name] = (out_len[0], len(block))
    print("pdict edge sizes (out, n):", sizes)
    # a period that starts in the dictionary goes on in the block: a few
    # sequences (and the 100 / 50 random bytes that end two of the blocks)
    for name in ("abc_across", "byte_across", "abc_last_20", "byte_last_7"):
        out, n = sizes[name]
        assert out < n // 4, (name, out, n)
    # the one source at distance 65535 is in reach (63 bytes for 4)
    out, n = sizes["dist65535"]
    assert out < n, (out, n)
    # and at 65536 it is not: 3064 random bytes do not compress
    out, n = sizes["dist65536"]
    assert out > n, (out, n)


def test_short_dictionary_gives_the_plain_bytes(gpu):
    """Below 4 bytes a dictionary holds no position: the bytes of
    compress_batch(table=PARSE_PARALLEL) without one."""
    buf = P.source("text", 200_000, seed=3)
    lens = (0, 1, 12, 13, 64, 100, 1000, 4096, 5000, 65536, 65537, 777)
    blocks, pos = [], 0
    for n in lens:
        blocks.append(buf[pos:pos + n])
        pos += n
    plain, plain_len = P.compress(blocks, None, gpu)
    assert plain_len[lens.index(65537)] == 0 and all(L > 0 for n, L in zip(lens, plain_len) if n <= 65536)
    for dl in (0, 1, 2, 3):
        got, got_len = P.compress(blocks, P.device_dict(b"the"[:dl], gpu), gpu)
        assert got_len == plain_len and got == plain, dl


def test_deterministic_and_batch_independent(gpu):
    import lz4.block
    buf = P.source("text", P.WINDOW + 200 * 1500, seed=4)
    D = buf[:P.WINDOW]
    blocks = [buf[P.WINDOW + 1500 * i: P.WINDOW + 1500 * (i + 1)] for i in range(200)]
    d = P.device_dict(D, gpu)
    first, _ = P.compress(blocks, d, gpu)
    again, _ = P.compress(blocks, d, gpu)
    assert first == again and all(c is not None for c in first)
    for k in (0, 57, 199):
        alone, _ = P.compress([blocks[k]], d, gpu)
        assert alone[0] == first[k], k
    prepared = lz4.block.prepare_dict(D)
    assert isinstance(prepared, lz4.block.PreparedDict) and prepared.dict_len == len(D)
    assert prepared.tail.numel() == P.WINDOW and prepared.table.numel() == 8192
    for _ in range(2):   # one preparation, two batches
        got, _ = P.compress(blocks, prepared, gpu)
        assert got == first
    # only the last 64 KiB count, whether the tensor or the PreparedDict holds more
    longer = b"\x07" * 1000 + D
    assert lz4.block.prepare_dict(longer).dict_len == len(longer)
    assert P.compress(blocks[:20], lz4.block.prepare_dict(longer), gpu)[0] == first[:20]
    assert P.compress(blocks[:20], P.device_dict(longer, gpu), gpu)[0] == first[:20]


def test_limited_output(gpu, oracle):
    rnd = P.source("random", 6 * 3000, seed=8)
    blocks = [rnd[3000 * i: 3000 * i + n] for i, n in enumerate((13, 64, 500, 1000, 2999, 3000))]
    D = P.source("text", 5000, seed=8)
    d = P.device_dict(D, gpu)
    # random bytes do not fit in n - 1: 0, and nothing written at or past the capacity (P.compress checks the guards)
    outs, out_len = P.compress(blocks, d, gpu, caps=[len(b) - 1 for b in blocks])
    assert out_len == [0] * len(blocks) and outs == [None] * len(blocks)
    # slots exactly as large as the output: accepted, the same bytes
    text = P.source("text", 40_000, seed=8)
    tb = [text[5000 + 2500 * i: 5000 + 2500 * (i + 1)] for i in range(12)] + [b"", b"x", text[:13]] + blocks[:2]
    free, free_len = P.compress(tb, d, gpu)
    assert all(L > 0 for L in free_len)
    exact, exact_len = P.compress(tb, d, gpu, caps=free_len)
    assert exact_len == free_len and exact == free
    P.check_decodes(oracle, tb, exact, D)
    # one byte less does not fit
    _, short_len = P.compress(tb, d, gpu, caps=[L - 1 for L in free_len])
    assert short_len == [0] * len(tb)


# total with the dictionary over the oracle's lz4.block.compress(dict=) total,
# measured on the MI355X and rounded up to the next 0.5 % (DESIGN.md section
# 3.8); the project's tolerance for this parse is 1.05 (test_parallel_parse_ratio)
BARS = {"text": 1.035, "source": 1.035, "markup": 0.975, "records": 0.985, "silesia": 0.99}


@pytest.mark.parametrize("kind", P.SIZE_KINDS)
def test_sizes_against_the_reference(gpu, oracle, kind):
    """The total of 32 x 4 KiB blocks with the 64 KiB before them as the
    dictionary stays within the measured bar of the oracle's
    lz4.block.compress(dict=) total (measured: text 76 426 / 74 045 = 1.0322,
    source 59 718 / 57 771 = 1.0337, markup 0.9715, records 0.9824, the mix
    0.9869), and on text, source and markup the dictionary pays: at most 0.95
    of the same parse without it (measured 0.805, 0.671, 0.799)."""
    D, blocks = P.size_case(kind)
    ref_plain = sum(len(oracle.compress(b)) for b in blocks)
    ref_dict = sum(len(oracle.compress_dict(b, D)) for b in blocks)
    assert (ref_plain, ref_dict) == P.ORACLE_TOTALS[kind]
    comps, out_len = P.compress(blocks, P.device_dict(D, gpu), gpu)
    P.check_decodes(oracle, blocks, comps, D)
    _, plain_len = P.compress(blocks, None, gpu)
    total, plain = sum(out_len), sum(plain_len)
    print(f"pdict sizes {kind}: dict {total} plain {plain} oracle dict {ref_dict} plain {ref_plain} "
          f"ratio {total / ref_dict:.4f} gain {total / plain:.4f}")
    bar = BARS[kind]
    assert bar <= 1.05
    assert total <= bar * ref_dict, (kind, total, ref_dict, total / ref_dict)
    if kind in ("text", "source", "markup"):   # the history must pay
        assert total <= 0.95 * plain, (kind, total, plain)


def test_compress_many_uploads_the_dictionary_once(gpu, oracle, monkeypatch):
    import lz4.block
    from lz4 import _native as N
    from lz4.block import _block as B
    D, blocks = P.size_case("source")
    staged = []
    real = B._stage_in

    def counting(dev, views, *a, **kw):
        staged.append(sum(v.nbytes for v in views))
        return real(dev, views, *a, **kw)

    uploads = []
    real_upload = N.to_device

    def counting_upload(buf, *a, **kw):
        uploads.append(memoryview(buf).nbytes)
        return real_upload(buf, *a, **kw)

    monkeypatch.setattr(B, "_stage_in", counting)
    monkeypatch.setattr(N, "to_device", counting_upload)
    comps = lz4.block.compress_many(blocks, dict=D, table=N.PARSE_PARALLEL, store_size=True)
    # the blocks alone are staged: no copy of the dictionary per block; the dictionary goes up once
    assert staged == [sum(len(b) for b in blocks)]
    assert uploads == [len(D)]
    monkeypatch.setattr(B, "_stage_in", real)
    monkeypatch.setattr(N, "to_device", real_upload)
    assert lz4.block.decompress_many(comps, dict=D) == blocks
    for b, c in zip(blocks[:4], comps[:4]):
        assert lz4.block.decompress(c, dict=D) == b
    bare = lz4.block.compress_many(blocks, dict=D, table=N.PARSE_PARALLEL, store_size=False)
    assert [c[4:] for c in comps] == bare
    assert all(int.from_bytes(c[:4], "little") == len(b) for b, c in zip(blocks, comps))
    batch, _ = P.compress(blocks, P.device_dict(D, gpu), gpu)
    assert bare == batch
    # a PreparedDict serves too, and only this combination takes one
    prepared = lz4.block.prepare_dict(D)
    assert lz4.block.compress_many(blocks, dict=prepared, table=N.PARSE_PARALLEL, store_size=False) == bare
    with pytest.raises(ValueError):
        lz4.block.compress_many(blocks, dict=prepared)
    # the default table keeps the exact dictionary parse
    exact = lz4.block.compress_many(blocks[:4], dict=D, store_size=False)
    assert exact == [oracle.compress_dict(b, D) for b in blocks[:4]]

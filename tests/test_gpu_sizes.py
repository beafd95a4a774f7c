"""GPU tests of the decoded-size pass (lz4m_decompressed_size_batch) and of
what is built on it: lz4.block.decompressed_size_batch / _many,
decompress_batch(dst_cap=None), decompress_many(uncompressed_size=None) and
lz4.frame.decompress_batch(direct=True).

The reference for a size is the CPU oracle's decoder at a capacity of
255 * len + 64, from which on its result no longer depends on the capacity;
for a decode at the exact size it is the oracle at that capacity.  Both walks
(a lane per block, a wavefront per block) must give the same values.
"""
import functools
import json
import os
import random
import struct

import numpy as np
import pytest
import torch

import layout_support as LS
import lz4.block
import lz4.frame
from lz4 import _native as N
from lz4 import _synth

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
WALKS = ["lane", "wave", "auto"]
POISON = 0x5A


def big_cap(c):
    return 255 * len(c) + 64


def _t(a, dtype, dev):
    return torch.tensor(np.asarray(a), dtype=dtype, device=dev)


def _pack(blobs, dev):
    """The blobs back to back on the device: (bytes, int64 offsets, int32 lengths)."""
    lens = [len(b) for b in blobs]
    off, _ = LS.plan_packed(lens)
    buf = torch.frombuffer(bytearray(b"".join(blobs) or b"\0"), dtype=torch.uint8).to(dev)
    return buf, _t(off, torch.int64, dev), _t(lens, torch.int32, dev)


def _sizes(blobs, dev, walk, dict_len=None):
    buf, off, ln = _pack(blobs, dev)
    dl = None if dict_len is None else _t(dict_len, torch.int32, dev)
    return lz4.block.decompressed_size_batch(buf, off, ln, dict_len=dl, walk=walk).cpu().tolist()


def _mismatches(got, want, blobs, limit=5):
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    return [(i, len(blobs[i]), got[i], want[i], blobs[i][:24].hex()) for i in bad[:limit]], len(bad)


# ------------------------------------------------------------ the case set
@functools.lru_cache(maxsize=None)
def _corpus():
    """The corpus of tests/test_gpu_layout.py (same seeds)."""
    blocks = [b.tobytes() for b in _synth.blocks(96, "silesia", seed=11)]
    rng = random.Random(5)
    sizes = [0, 1, 4, 5, 11, 12, 13, 14, 15, 16, 17, 31, 32, 63, 64, 65, 100, 255, 256, 1000, 4095, 4096,
             65535, 65536]
    return blocks, [blocks[rng.randrange(len(blocks))][:s] for s in sizes]


def _golden_decode_vectors():
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    arr = np.load(os.path.join(GOLDEN, "golden.npz"), allow_pickle=False)
    return [arr[e["key"]].tobytes() for e in man["decompress"]]


@pytest.fixture(scope="module")
def case_set(oracle):
    """The ingredients of test_gpu_layout.edge_cases, each distinct block once:
    (blocks, the oracle's status at a capacity that does not matter)."""
    blocks, ragged = _corpus()
    blobs = [oracle.compress(b) for b in ragged + blocks[:8] + LS._long_sequence_blocks(4, 41)]
    wl, _caps, valid = LS.whole_literal_cases()
    blobs += wl + [b for b, _ in valid]
    blobs += LS.malformed_cases(oracle, blocks, count=600)[0]
    blobs += LS.offset0_cases(64)[0]
    blobs += _golden_decode_vectors()
    blobs = list(dict.fromkeys(blobs))
    want = [oracle.decompress(c, big_cap(c))[0] for c in blobs]
    assert sum(w < 0 for w in want) >= 100 and sum(w >= 0 for w in want) >= 300
    return blobs, want


# ------------------------------------------------------------ 1. statuses
@pytest.mark.parametrize("walk", WALKS)
def test_statuses_equal_the_oracle(gpu, case_set, walk):
    blobs, want = case_set
    got = _sizes(blobs, gpu, walk)
    bad, nbad = _mismatches(got, want, blobs)
    assert nbad == 0, (walk, nbad, bad)


# ------------------------------------------------------------ 2. containment
@pytest.mark.parametrize("walk", WALKS)
def test_only_the_size_words_change_under_a_scattered_layout(gpu, case_set, walk):
    """The blocks in a shuffled order between 0xFF bytes, the sizes inside a
    poisoned buffer: only the n size words change, and they are those of the
    packed layout."""
    blobs, want = case_set
    n = len(blobs)
    alloc, src_off = LS.plan_sources(blobs, seed=9)
    src = torch.from_numpy(alloc).to(gpu)[1:]
    pad = 37   # words of poison before and after
    words = torch.full((n + 2 * pad,), POISON * 0x01010101, dtype=torch.int32, device=gpu)
    N.launch_decompressed_size(src, _t(src_off, torch.int64, gpu), _t([len(b) for b in blobs], torch.int32, gpu),
                               words[pad:pad + n], n, walk=walk)
    host = words.cpu().numpy()
    LS.assert_outside_intact(host.view(np.uint8), [4 * pad], [4 * n], POISON, walk)
    got = host[pad:pad + n].tolist()
    bad, nbad = _mismatches(got, want, blobs)
    assert nbad == 0, (walk, nbad, bad)


# ------------------------------------------------------------ 3. window edges
def _window_blocks(oracle):
    """Blocks whose sequences straddle the wave walk's staging (1 KiB refills
    of a 2 KiB ring, 64 start bytes a round) and the lane walk's 64-byte
    refills: an incompressible head of every length moves a 3 000-byte
    literal, a match-length run of 40 length bytes and the tokens after them
    across every boundary; hand-written runs of 4-byte sequences put a token
    on every byte near a refill."""
    rng = np.random.default_rng(31)
    noise = rng.integers(0, 256, 8192, dtype=np.uint8).tobytes()
    text = _corpus()[0][3][:600]
    out = []
    for k in list(range(0, 70)) + list(range(930, 1100, 1)) + list(range(1990, 2070, 3)):
        data = (noise[:k] + text[:200] + text[:120] + noise[4000:7000] + text[100:300] + bytes(40 * 255 + 30) +
                noise[100:120] + text[:64] + b"tail!tail!")
        out.append(oracle.compress(data))
    for lead in range(0, 16):
        seqs = LS.lz4_sequence(noise[:lead + 1], 1, 4)
        for j in range(560):   # tokens at every fourth byte up to ~2.2 KiB: lit 1, match 4..19 or a one-byte run
            seqs += LS.lz4_sequence(noise[j:j + 1], 1 + j % 5, 4 + (j * 7) % 30)
        out.append(seqs + LS.lz4_sequence(b"final"))
    return out


@pytest.mark.parametrize("walk", ["lane", "wave"])
def test_sequences_across_staging_windows(gpu, oracle, walk):
    blobs = _window_blocks(oracle)
    want = [oracle.decompress(c, big_cap(c))[0] for c in blobs]
    assert all(w > 0 for w in want)
    got = _sizes(blobs, gpu, walk)
    bad, nbad = _mismatches(got, want, blobs)
    assert nbad == 0, (walk, nbad, bad)


# ------------------------------------------------------------ 4. large blocks
def _frame_payloads(frame):
    """(payload, stored) of every block record of a frame's bytes."""
    flg = frame[4]
    pos = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    out = []
    while True:
        h = struct.unpack_from("<I", frame, pos)[0]
        pos += 4
        if h == 0:
            return out
        ln = h & 0x7FFFFFFF
        out.append((frame[pos:pos + ln], bool(h >> 31)))
        pos += ln + (4 if flg & 16 else 0)


@pytest.fixture(scope="module")
def large_blocks(gpu):
    data = b"".join(b.tobytes() for b in _synth.blocks(80, "silesia", seed=3))   # 5 MiB: blocks of 4 and 1 MiB
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(gpu)
    frame = lz4.frame.compress_device(t, len(data), parse="parallel", block_size=lz4.frame.BLOCKSIZE_MAX4MB,
                                      block_linked=False).cpu().numpy().tobytes()
    recs = _frame_payloads(frame)
    assert [s for _, s in recs] == [False, False]
    return [p for p, _ in recs]


@pytest.mark.parametrize("walk", ["lane", "wave"])
def test_large_blocks(gpu, large_blocks, walk):
    assert _sizes(large_blocks, gpu, walk) == [4 << 20, 1 << 20]


# ------------------------------------------------------------ 5. overflow
def _long_match_block(k, last=0):
    """Token 0x1F, one literal, offset 1, k length bytes of 255 and `last`, then five last literals."""
    return b"\x1fa\x01\x00" + b"\xff" * k + bytes([last]) + b"\x50tail!"


@pytest.mark.parametrize("walk", ["lane", "wave"])
def test_size_overflow(gpu, walk):
    k = 8_421_505   # 15 + 4 + 255 k alone is above INT32_MAX
    assert 19 + 255 * k > 2**31 - 1 >= 1 + 19 + 255 * (k - 1000) + 7 + 5
    blobs = [_long_match_block(k), _long_match_block(k - 1000, 7)]
    assert _sizes(blobs, gpu, walk) == [N.SIZE_OVERFLOW, 1 + (15 + 4 + 255 * (k - 1000) + 7) + 5]


# ------------------------------------------------------------ 6. dictionary
@pytest.fixture(scope="module")
def dict_cases(oracle):
    """(blocks, their dictionaries, dictionary index per block): blocks that
    start with bytes of their dictionary, so that the first match reaches
    into it, for dictionaries of 1, 100, 65 535 and 70 000 bytes."""
    blocks, _ = _corpus()
    pool = b"".join(blocks[20:22])
    dicts = [pool[-n:] for n in (1, 100, 65535, 70000)]
    blobs, which = [], []
    for d, dd in enumerate(dicts):
        for j, size in enumerate((40, 700, 5000, 65536)):
            data = (dd[-min(len(dd), 300):] + blocks[30 + j] + dd[:min(len(dd), 200)])[:size]
            blobs.append(oracle.compress_dict(data, dd))
            which.append(d)
    return blobs, dicts, which


@pytest.mark.parametrize("walk", WALKS)
def test_dictionary_lengths(gpu, oracle, dict_cases, walk):
    blobs, dicts, which = dict_cases
    with_dict = [oracle.decompress(c, big_cap(c), dict_=dicts[d])[0] for c, d in zip(blobs, which)]
    without = [oracle.decompress(c, big_cap(c))[0] for c in blobs]
    assert all(w > 0 for w in with_dict) and sum(w < 0 for w in without) >= 8
    assert _sizes(blobs, gpu, walk, [len(dicts[d]) for d in which]) == with_dict
    assert _sizes(blobs, gpu, walk, [0] * len(blobs)) == without
    assert _sizes(blobs, gpu, walk) == without


# ------------------------------------------------------------ 7. decompress_batch(dst_cap=None)
def _check_exact_decode(gpu, oracle, blobs, sizes, dicts=None, which=None):
    n = len(blobs)
    buf, off, ln = _pack(blobs, gpu)
    kw = {}
    if dicts is not None:
        d_off, _ = LS.plan_packed([len(d) for d in dicts])
        kw = dict(dict_buf=torch.frombuffer(bytearray(b"".join(dicts)), dtype=torch.uint8).to(gpu),
                  dict_off=_t([d_off[d] for d in which], torch.int64, gpu),
                  dict_len=_t([len(dicts[d]) for d in which], torch.int32, gpu))
    total = sum(max(s, 0) for s in sizes)
    dst, dst_off, status = lz4.block.decompress_batch(buf, off, ln, **kw)
    assert dst.numel() == max(total, 1)
    room = torch.full((total + LS.TAIL,), POISON, dtype=torch.uint8, device=gpu)
    dst2, dst_off2, status2 = lz4.block.decompress_batch(buf, off, ln, dst=room, **kw)
    assert dst2 is room and torch.equal(dst_off, dst_off2) and torch.equal(status, status2)
    host = room.cpu().numpy()
    assert (host[total:] == POISON).all()
    caps = [max(s, 0) for s in sizes]
    want_off, _ = LS.plan_packed(caps)
    assert dst_off.cpu().tolist() == want_off.tolist()
    st = status.cpu().tolist()
    first = dst.cpu().numpy()
    needs_slack = 0
    for i, c in enumerate(blobs):
        if sizes[i] < 0:
            assert st[i] == sizes[i], (i, st[i], sizes[i])
            continue
        w, data = oracle.decompress(c, sizes[i], dict_=None if dicts is None else dicts[which[i]])
        assert st[i] == w, (i, len(c), sizes[i], st[i], w)
        needs_slack += w < 0
        if w >= 0:
            o = int(want_off[i])
            assert host[o:o + w].tobytes() == data and first[o:o + w].tobytes() == data, i
    return needs_slack


def test_decompress_batch_without_capacities(gpu, oracle, case_set):
    blobs, sizes = case_set
    _check_exact_decode(gpu, oracle, blobs, sizes)


def test_decompress_batch_without_capacities_with_dictionaries(gpu, oracle, dict_cases):
    blobs, dicts, which = dict_cases
    sizes = [oracle.decompress(c, big_cap(c), dict_=dicts[d])[0] for c, d in zip(blobs, which)]
    _check_exact_decode(gpu, oracle, blobs, sizes, dicts, which)


# ------------------------------------------------------------ 8. host forms
def test_decompress_many_with_unknown_sizes(gpu, oracle):
    _, ragged = _corpus()
    comp = lz4.block.compress_many(ragged, store_size=False)
    assert lz4.block.decompress_many(comp, uncompressed_size=None) == ragged
    assert lz4.block.decompressed_size_many(comp) == [len(b) for b in ragged]
    hdr = lz4.block.compress_many(ragged, store_size=True)
    kinds = [None, "len", -1]
    mixed = [(comp[i], None) if kinds[i % 3] is None else (comp[i], len(ragged[i])) if kinds[i % 3] == "len"
             else (hdr[i], -1) for i in range(len(ragged))]
    assert lz4.block.decompress_many([b for b, _ in mixed], uncompressed_size=[s for _, s in mixed]) == ragged
    got = lz4.block.decompress_many(comp, uncompressed_size=None, as_bytearray=True)
    assert all(type(g) is bytearray for g in got) and [bytes(g) for g in got] == ragged
    # a malformed block: raised, or returned in its slot
    bad = comp[-1][:len(comp[-1]) // 2]
    st = oracle.decompress(bad, big_cap(bad))[0]
    assert st < 0
    msg = f"Decompression failed: corrupt input or insufficient space in destination buffer. Error code: {-st}"
    with pytest.raises(lz4.block.LZ4BlockError) as e:
        lz4.block.decompress_many([comp[3], bad, comp[5]], uncompressed_size=None)
    assert str(e.value) == msg
    res = lz4.block.decompress_many([comp[3], bad, comp[5]], uncompressed_size=None, raise_errors=False)
    assert res[0] == ragged[3] and res[2] == ragged[5]
    assert isinstance(res[1], lz4.block.LZ4BlockError) and str(res[1]) == msg
    with pytest.raises(lz4.block.LZ4BlockError) as e:
        lz4.block.decompressed_size_many([comp[3], bad])
    assert str(e.value) == msg
    assert lz4.block.decompressed_size_many([comp[3], bad], raise_errors=False) == [len(ragged[3]), st]
    # with a dictionary
    d = _corpus()[0][40][:5000]
    src = [d[-200:] + b[:3000] for b in _corpus()[0][:6]]
    cd = lz4.block.compress_many(src, store_size=False, dict=d)
    assert lz4.block.decompress_many(cd, uncompressed_size=None, dict=d) == src
    assert lz4.block.decompressed_size_many(cd, dict=d) == [len(s) for s in src]
    assert lz4.block.decompress_many([], uncompressed_size=None) == [] and lz4.block.decompressed_size_many([]) == []


# ------------------------------------------------------------ 9. frames
import test_gpu_frame_batch as FB   # noqa: E402  the frame sets of the batched frame tests


def _both(gpu, frames):
    buf, off, ln = FB._pack(gpu, frames)
    a = lz4.frame.decompress_batch(buf, off, ln)
    b = lz4.frame.decompress_batch(buf, off, ln, direct=True)
    return a, b


def _assert_same(a, b, what):
    for name, x, y in zip(("out", "out_off", "out_len", "status", "bytes_read"), a, b):
        assert x.dtype == y.dtype and torch.equal(x, y), (what, name)


def _golden_frames():
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    arr = np.load(os.path.join(GOLDEN, "golden.npz"), allow_pickle=False)
    return [arr[e["key"]].tobytes() for e in man["frames"]]


@pytest.mark.parametrize("linked,cc,bc", [(True, True, True), (False, True, False), (False, False, True),
                                          (True, False, False)])
def test_direct_equals_slots_on_mixed_batches(gpu, linked, cc, bc):
    items = FB._mixed()[:96]
    frames = lz4.frame.compress_many(items, block_linked=linked, content_checksum=cc, block_checksum=bc)
    a, b = _both(gpu, frames)
    assert a[3].cpu().tolist() == [0] * len(frames) and FB._cut(a[0], a[1], a[2]) == items
    _assert_same(a, b, (linked, cc, bc))


def test_direct_equals_slots_on_every_block_size(gpu):
    text = FB._streams()["text"]
    frames = []
    for bsid in (4, 5, 6, 7):
        frames += lz4.frame.compress_many([text[:300_000], text[:70_000], b""], block_size=bsid, block_linked=False,
                                          content_checksum=True)
        frames += lz4.frame.compress_many([text[:300_000]], block_size=bsid, block_linked=True)
    frames += lz4.frame.compress_many(FB._big_batch(), block_size=7, block_linked=False, block_checksum=True)
    a, b = _both(gpu, frames)
    assert a[3].cpu().tolist() == [0] * len(frames)
    _assert_same(a, b, "block sizes")


def test_direct_equals_slots_on_hand_built_corrupt_and_golden_frames(gpu):
    hand = [f for _, f, _ in FB._hand_built()]
    corrupt = [f for _, f in FB._corrupt_cases()]
    good = lz4.frame.compress_many([FB._distinct()[i] for i in (7, 6, 0, 15, 5, 22)], block_linked=False,
                                   content_checksum=True)
    frames = []
    for i, f in enumerate(corrupt):   # every bad frame between good ones
        frames += [good[i % len(good)], f]
    frames += hand + _golden_frames()
    a, b = _both(gpu, frames)
    st = a[3].cpu().tolist()
    assert all(st[2 * i] == 0 and st[2 * i + 1] != 0 for i in range(len(corrupt)))
    assert st[2 * len(corrupt):] == [0] * (len(frames) - 2 * len(corrupt))
    _assert_same(a, b, "hand-built, corrupt, golden")


def test_direct_allocates_no_slots_for_independent_frames(gpu):
    nfr, bs = 256, 65536
    text = FB._streams()["text"]
    items = [text[(997 * i) % 60_000:][:bs] for i in range(nfr)]
    buf, off, ln = FB._pack(gpu, items)
    frames, f_off, f_len = lz4.frame.compress_batch(buf, off, ln, block_linked=False)
    peak = {}
    for direct in (False, True, False, True):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = lz4.frame.decompress_batch(frames, f_off, f_len, direct=direct)
        torch.cuda.synchronize()
        peak[direct] = torch.cuda.max_memory_allocated() - base
        assert res[3].cpu().tolist() == [0] * nfr
        if direct:
            assert FB._cut(res[0], res[1], res[2]) == items
        del res
    print(f"peak allocated bytes: slots {peak[False]}, direct {peak[True]}, blocks x block size {nfr * bs}")
    assert peak[False] - peak[True] >= nfr * bs // 2, peak


def test_direct_fails_a_block_that_needs_slack(gpu, oracle):
    """Eight literals, a match of four that starts 9 bytes before the end,
    five last literals: it decodes at any capacity of 20 bytes or more and
    not at its size, 17 (the reference wants 12 bytes after the last match's
    start, lz4.c:2172-2229)."""
    blk = LS.lz4_sequence(b"abcdefgh", 8, 4) + LS.lz4_sequence(b"tail!")
    assert oracle.decompress(blk, big_cap(blk))[0] == 17 == oracle.decompress(blk, 65536)[0]
    assert oracle.decompress(blk, 17)[0] < 0
    ok = lz4.block.compress(b"an ordinary block " * 40, store_size=False)
    frames = [FB._frame([(ok, 0), (blk, 0)]), FB._frame([(ok, 0)])]
    assert lz4.frame.decompress(frames[0]) == b"an ordinary block " * 40 + b"abcdefghabcdtail!"
    a, b = _both(gpu, frames)
    assert a[3].cpu().tolist() == [0, 0]
    assert b[3].cpu().tolist() == [N.FRAME_BLOCK_FAILED, 0]
    assert FB._cut(b[0], b[1], b[2])[1] == b"an ordinary block " * 40

"""GPU tests of the batched frame calls: lz4.frame.compress_many /
decompress_many (host bytes), compress_batch / decompress_batch (device
tensors) and lz4m_decompress_chains.

The reference behaviour is what this file does not change: the golden frames
the reference wrote (tests/golden), the single-frame calls (pinned to the
reference by tests/test_gpu_api.py) and lz4.block, used to hand-build frames
the compressor never writes.

Inputs: 0, 1, 12, 13, 65535, 65536, 65537 and 131077 bytes at 64 KiB blocks
(an empty frame, a one-literal-run block, a single full block -- never
linked --, the first linked frame, a short last block), and one frame of
4 MiB + 1 bytes in a batch compressed at block-size id 7, in which every other
frame's id is lowered by the optimal rule; text, random and runs."""
import functools
import itertools
import json
import os
import random
import struct

import numpy as np
import pytest

import lz4.block
import lz4.frame
from lz4 import _synth

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        man = json.load(f)
    return man, np.load(os.path.join(GOLDEN, "golden.npz"), allow_pickle=False)


def _b(arr, key):
    return arr[key].tobytes()


SIZES =[0, 1, 12, 13, 65535, 65536, 65537, 131077]
KINDS = ["text", "random", "runs"]
BIG = (4 << 20) + 1


@functools.lru_cache(maxsize=None)
def _streams():
    rng = np.random.default_rng(77)
    return {k: _synth.KINDS[k](rng, 3 * 131077).tobytes() for k in KINDS}


@functools.lru_cache(maxsize=None)
def _distinct():
    """The 24 distinct inputs (kind x size), each a different cut of its kind's stream."""
    out = []
    for k in KINDS:
        s = _streams()[k]
        for j, size in enumerate(SIZES):
            start = 1000 * j
            out.append(s[start:start + size])
    return out


@functools.lru_cache(maxsize=None)
def _mixed():
    """192 inputs: every distinct input eight times, shuffled, so that linked, independent and empty frames
    interleave."""
    items = _distinct() * 8
    random.Random(5).shuffle(items)
    return items


@functools.lru_cache(maxsize=None)
def _big_batch():
    """The batch compressed at block-size id 7: the 4 MiB + 1 frame (two linked blocks) among one input of each
    size, whose ids the optimal rule lowers."""
    rng = np.random.default_rng(78)
    big = _synth.word_text(rng, BIG).tobytes()
    items = list(_distinct()[:8])
    return items[:4] + [big] + items[4:]


_SINGLE = {}


def _single(data, **opts):
    """lz4.frame.compress of one input, computed once per (input, options)."""
    key = (data, tuple(sorted(opts.items())))
    if key not in _SINGLE:
        _SINGLE[key] = lz4.frame.compress(data, **opts)
    return _SINGLE[key]


def _pack(gpu, items):
    import torch
    lens = [len(x) for x in items]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if items else np.zeros(0, np.int64)
    buf = torch.frombuffer(bytearray(b"".join(items) or b"\0"), dtype=torch.uint8).to(gpu)
    if not sum(lens):
        buf = buf[:0]
    return buf, torch.tensor(offs, dtype=torch.int64, device=gpu), torch.tensor(lens, dtype=torch.int64, device=gpu)


def _cut(buf, off, length):
    h = buf.cpu().numpy()
    return [h[o:o + n].tobytes() for o, n in zip(off.cpu().tolist(), length.cpu().tolist())]


def _assert_back_to_back(buf, off, length):
    """Capacity: the spans lie inside the buffer, in order, without overlap -- and, as both calls pack their
    results, without a gap, so there is no byte outside a span to write to."""
    o, n = off.cpu().tolist(), length.cpu().tolist()
    pos = 0
    for a, b in zip(o, n):
        assert a == pos and b >= 0
        pos = a + b
    assert pos == buf.numel()


def _kw(o):
    return dict(block_size=o["block_size_id"], block_linked=bool(o.get("linked")),
                content_checksum=o.get("content_checksum", True), block_checksum=o.get("block_checksum", False),
                store_size=o.get("store_size", True), compression_level=o.get("level", 0))


# ------------------------------------------------------------ golden frames
def test_golden_frames_compress(gpu, golden):
    man, arr = golden
    inputs = {e["name"]: _b(arr, e["key"]) for e in man["inputs"]}
    groups = {}
    for e in man["frames"]:
        groups.setdefault(tuple(sorted(_kw(e["opts"]).items())), []).append(e)
    nlinked = 0
    for key, entries in groups.items():
        kw = dict(key)
        datas = [inputs[e["input"]] for e in entries]
        want = [_b(arr, e["key"]) for e in entries]
        nlinked += len(entries) * bool(kw["block_linked"])
        assert lz4.frame.compress_many(datas, **kw) == want, kw
        buf, off, ln = _pack(gpu, datas)
        frames, f_off, f_len = lz4.frame.compress_batch(buf, off, ln, **kw)
        assert _cut(frames, f_off, f_len) == want, kw
    assert nlinked >= 4


def test_golden_frames_in_one_batch_per_linking(gpu, golden):
    """The golden frames that differ only in their input share a call: all inputs through each option set, each
    result equal to the single call (the manifest has one frame per option set)."""
    man, arr = golden
    inputs = [_b(arr, e["key"]) for e in man["inputs"]][:24]
    for e in man["frames"][:4]:
        kw = _kw(e["opts"])
        assert lz4.frame.compress_many(inputs, **kw) == [_single(d, **kw) for d in inputs]


@pytest.mark.parametrize("junk", [0, 7])
def test_golden_frames_decode(gpu, golden, junk):
    import torch
    man, arr = golden
    inputs = {e["name"]: _b(arr, e["key"]) for e in man["inputs"]}
    frames = [_b(arr, e["key"]) for e in man["frames"]]
    want = [inputs[e["input"]] for e in man["frames"]]
    tail = bytes(range(0xF9, 0xF9 + junk))
    padded = [f + tail for f in frames]
    assert lz4.frame.decompress_many(padded) == want
    got = lz4.frame.decompress_many(padded, return_bytes_read=True, return_bytearray=True)
    assert [(bytes(a), b) for a, b in got] == [(w, len(f)) for w, f in zip(want, frames)]
    assert all(type(a) is bytearray for a, _ in got)
    buf, off, ln = _pack(gpu, padded)
    out, o_off, o_len, status, read = lz4.frame.decompress_batch(buf, off, ln)
    assert status.dtype == torch.int32 and status.cpu().tolist() == [0] * len(frames)
    assert read.cpu().tolist() == [len(f) for f in frames]
    assert _cut(out, o_off, o_len) == want
    _assert_back_to_back(out, o_off, o_len)


# ------------------------------------------------- mixed batch = single call
GRID = list(itertools.product([True, False], repeat=4))


@pytest.mark.parametrize("linked,cc,bc,ss", GRID, ids=["".join("LCBS"[i] if v else "-" for i, v in enumerate(g))
                                                        for g in GRID])
def test_mixed_batch_equals_single_calls(gpu, linked, cc, bc, ss):
    kw = dict(block_linked=linked, content_checksum=cc, block_checksum=bc, store_size=ss)
    items = _mixed()
    got = lz4.frame.compress_many(items, **kw)
    assert len(got) == len(items)
    for i, (g, d) in enumerate(zip(got, items)):
        assert g == _single(d, **kw), (i, len(d))
    assert lz4.frame.decompress_many(got) == items


@pytest.mark.parametrize("linked,cc,bc,ss", GRID[::5], ids=["".join("LCBS"[i] if v else "-" for i, v in enumerate(g))
                                                             for g in GRID[::5]])
def test_block_size_7_batch_equals_single_calls(gpu, linked, cc, bc, ss):
    """The 4 MiB + 1 frame at block-size id 7 (two blocks, linked when asked) among frames whose id is lowered."""
    kw = dict(block_size=lz4.frame.BLOCKSIZE_MAX4MB, block_linked=linked, content_checksum=cc, block_checksum=bc,
              store_size=ss)
    items = _big_batch()
    got = lz4.frame.compress_many(items, **kw)
    for i, (g, d) in enumerate(zip(got, items)):
        assert g == _single(d, **kw), (i, len(d))
    ids = [lz4.frame.get_frame_info(g)["block_size_id"] for g in got]
    assert ids[4] == 7 and set(ids[:4]) == {4} and ids[-1] == 5
    assert lz4.frame.get_frame_info(got[4])["block_linked"] == linked
    assert lz4.frame.decompress_many(got) == items


def _device_singles(gpu, items, **kw):
    import torch
    out = []
    for d in items:
        t = torch.frombuffer(bytearray(d or b"\0"), dtype=torch.uint8).to(gpu)
        out.append(lz4.frame.compress_device(t, len(d), **kw).cpu().numpy().tobytes())
    return out


@pytest.mark.parametrize("linked", [True, False])
def test_mixed_batch_hc_equals_compress_device(gpu, linked):
    kw = dict(parse="hc", compression_level=4, block_linked=linked, content_checksum=True)
    distinct = _distinct()
    want = dict(zip(distinct, _device_singles(gpu, distinct, **kw)))
    items = _mixed()[:96]
    buf, off, ln = _pack(gpu, items)
    frames, f_off, f_len = lz4.frame.compress_batch(buf, off, ln, **kw)
    got = _cut(frames, f_off, f_len)
    for i, (g, d) in enumerate(zip(got, items)):
        assert g == want[d], (i, len(d))
    assert lz4.frame.decompress_many(got) == items


def test_block_size_7_batch_hc_equals_compress_device(gpu):
    kw = dict(parse="hc", compression_level=4, block_size=7, content_checksum=True)
    items = _big_batch()
    buf, off, ln = _pack(gpu, items)
    frames, f_off, f_len = lz4.frame.compress_batch(buf, off, ln, **kw)
    got = _cut(frames, f_off, f_len)
    assert got == _device_singles(gpu, items, **kw)
    assert lz4.frame.decompress_many(got) == items


@pytest.mark.parametrize("block_size", [0, 7])
def test_mixed_batch_parallel_parse_round_trips(gpu, block_size):
    items = _mixed()[:96] if block_size == 0 else _big_batch()
    buf, off, ln = _pack(gpu, items)
    frames, f_off, f_len = lz4.frame.compress_batch(buf, off, ln, parse="parallel", block_size=block_size,
                                                    content_checksum=True, block_checksum=True)
    _assert_back_to_back(frames, f_off, f_len)
    out, o_off, o_len, status, read = lz4.frame.decompress_batch(frames, f_off, f_len)
    assert status.cpu().tolist() == [0] * len(items)
    assert read.cpu().tolist() == f_len.cpu().tolist()
    assert _cut(out, o_off, o_len) == items
    for f, d in zip(_cut(frames, f_off, f_len)[:12], items):
        assert lz4.frame.decompress(f) == d


# ------------------------------------------------------- batch independence
def test_a_frame_does_not_depend_on_its_batch(gpu):
    kw = dict(content_checksum=True, block_checksum=True)
    items = _mixed()
    sizes = [len(d) for d in items]
    chosen = [sizes.index(0), sizes.index(13), sizes.index(65536), sizes.index(65537), sizes.index(131077)]
    buf, off, ln = _pack(gpu, items)
    frames, f_off, f_len = lz4.frame.compress_batch(buf, off, ln, **kw)
    all_frames = _cut(frames, f_off, f_len)
    out, o_off, o_len, status, read = lz4.frame.decompress_batch(frames, f_off, f_len)
    all_out = _cut(out, o_off, o_len)
    assert all_out == items
    for i in chosen:
        one, one_off, one_len = lz4.frame.compress_batch(buf, off[i:i + 1], ln[i:i + 1], **kw)
        assert _cut(one, one_off, one_len) == [all_frames[i]]
        o1, o1_off, o1_len, st1, rd1 = lz4.frame.decompress_batch(frames, f_off[i:i + 1], f_len[i:i + 1])
        assert _cut(o1, o1_off, o1_len) == [all_out[i]]
        assert st1.cpu().tolist() == [0] and rd1.cpu().tolist() == [len(all_frames[i])]


# ------------------------------------------------------- hand-built frames
def _hc_byte(desc: bytes) -> bytes:
    from lz4 import _native as N
    return bytes([(N.xxh32_host(desc) >> 8) & 0xFF])


def _frame(blocks, *, linked=False, size=None, dict_id=None, bsid=4, endmark=True):
    """A frame from (payload, stored) pairs: header, records, endmark; no checksums."""
    flg = (1 << 6) | ((0 if linked else 1) << 5) | ((size is not None) << 3) | (dict_id is not None)
    desc = bytes([flg, bsid << 4])
    if size is not None:
        desc += struct.pack("<Q", size)
    if dict_id is not None:
        desc += struct.pack("<I", dict_id)
    out = struct.pack("<I", 0x184D2204) + desc + _hc_byte(desc)
    for payload, stored in blocks:
        out += struct.pack("<I", len(payload) | (0x80000000 if stored else 0)) + payload
    return out + (struct.pack("<I", 0) if endmark else b"")


def _blk(data, history=b""):
    if history:
        return lz4.block.compress(data, store_size=False, dict=history[-65536:])
    return lz4.block.compress(data, store_size=False)


@functools.lru_cache(maxsize=None)
def _hand_built():
    """(name, frame bytes, content or None when decompress must tell) of frames LZ4F_compressFrame never writes."""
    t = _streams()["text"]
    a, b, c = t[:1000], t[500:2500], t[2000:5000]   # overlapping cuts: later blocks match earlier ones
    rnd = _streams()["random"][:700]
    return [
        ("short non-final block, independent", _frame([(_blk(a), 0), (_blk(b), 0), (_blk(c), 0)]), a + b + c),
        ("short non-final block, linked",
         _frame([(_blk(a), 0), (_blk(b, a), 0), (_blk(c, a + b), 0)], linked=True), a + b + c),
        ("stored block mid-frame, independent", _frame([(_blk(a), 0), (rnd, 1), (_blk(c), 0)]), a + rnd + c),
        ("stored block mid-frame, linked",
         _frame([(_blk(a), 0), (rnd, 1), (_blk(c, a + rnd), 0), (_blk(a, a + rnd + c), 0)], linked=True),
         a + rnd + c + a),
        ("stored blocks only, linked", _frame([(rnd, 1), (a, 1)], linked=True), rnd + a),
        ("no content size", _frame([(_blk(c), 0)]), c),
        ("content size", _frame([(_blk(a), 0), (_blk(b), 0)], size=len(a + b)), a + b),
        ("dict id", _frame([(_blk(a), 0), (_blk(b, a), 0)], linked=True, dict_id=0x12345678, size=len(a + b)), a + b),
        ("skippable", struct.pack("<II", 0x184D2A53, 11) + b"hello world", b""),
        ("empty skippable", struct.pack("<II", 0x184D2A50, 0), b""),
        ("no blocks", _frame([]), b""),
    ]


def test_hand_built_frames_decode_as_the_single_call(gpu):
    cases = _hand_built()
    frames = [f for _, f, _ in cases]
    single = [lz4.frame.decompress(f, return_bytes_read=True) for f in frames]
    for (name, f, want), (got, read) in zip(cases, single):
        assert got == want and read == len(f), name          # the single call agrees with the construction
    assert lz4.frame.decompress_many(frames, return_bytes_read=True) == single
    buf, off, ln = _pack(gpu, frames)
    out, o_off, o_len, status, read = lz4.frame.decompress_batch(buf, off, ln)
    assert status.cpu().tolist() == [0] * len(frames)
    assert _cut(out, o_off, o_len) == [w for _, _, w in cases]
    assert read.cpu().tolist() == [len(f) for f in frames]
    _assert_back_to_back(out, o_off, o_len)


def test_concatenated_frames_by_bytes_read(gpu):
    import torch
    cases = _hand_built()
    f1, w1 = cases[1][1], cases[1][2]
    f2, w2 = lz4.frame.compress(_distinct()[7], content_checksum=True), _distinct()[7]
    both = f1 + f2
    buf, off, ln = _pack(gpu, [both])
    out, o_off, o_len, status, read = lz4.frame.decompress_batch(buf, off, ln)
    assert status.cpu().tolist() == [0] and read.cpu().tolist() == [len(f1)]
    assert lz4.frame.decompress(both, return_bytes_read=True) == (w1, len(f1))
    off2 = torch.cat([off, read])
    ln2 = torch.cat([ln, ln - read])
    out, o_off, o_len, status, read = lz4.frame.decompress_batch(buf, off2, ln2)
    assert status.cpu().tolist() == [0, 0] and read.cpu().tolist() == [len(f1), len(f2)]
    assert _cut(out, o_off, o_len) == [w1, w2]


# ------------------------------------------------- errors stay local, match
def _patch(frame, pos, fn):
    b = bytearray(frame)
    b[pos] = fn(b[pos]) & 0xFF
    return bytes(b)


@functools.lru_cache(maxsize=None)
def _corrupt_cases():
    d = _distinct()[7]             # 131077 bytes of text: three blocks
    plain = lz4.frame.compress(d, store_size=False)                      # header 7 bytes
    sized = lz4.frame.compress(d)                                        # header 15 bytes
    cc = lz4.frame.compress(d, content_checksum=True, store_size=False)
    bc = lz4.frame.compress(d, block_checksum=True, store_size=False)
    first = struct.unpack_from("<I", plain, 7)[0] & 0x7FFFFFFF
    wrong_size = bytearray(sized)
    struct.pack_into("<Q", wrong_size, 6, len(d) + 1)
    wrong_size[14:15] = _hc_byte(bytes(wrong_size[4:14]))
    too_large = bytearray(plain)
    struct.pack_into("<I", too_large, 7, 65537)
    return [
        ("truncated header", plain[:5]),
        ("truncated header, sized", sized[:12]),
        ("truncated block", plain[:7 + 4 + first // 2]),
        ("missing endmark", plain[:-4]),
        ("missing endmark and content checksum", cc[:-8]),
        ("missing content checksum", cc[:-3]),
        ("flipped header checksum", _patch(plain, 6, lambda v: v ^ 0xFF)),
        ("reserved FLG bit", _patch(plain, 4, lambda v: v | 0x02)),
        ("reserved BD bit", _patch(plain, 5, lambda v: v | 0x80)),
        ("wrong version", _patch(plain, 4, lambda v: v | 0x80)),
        ("unknown magic", _patch(plain, 0, lambda v: v ^ 0x01)),
        ("block-size id 3", _patch(plain, 5, lambda v: 0x30)),
        ("flipped payload byte, block checksum", _patch(bc, 7 + 4 + 40, lambda v: v ^ 0x10)),
        ("flipped payload byte, content checksum", _patch(cc, 7 + 4 + 40, lambda v: v ^ 0x10)),
        ("undecodable payload", plain[:11] + b"\xff" * first + plain[11 + first:]),
        ("flipped content checksum", _patch(cc, len(cc) - 1, lambda v: v ^ 0x01)),
        ("wrong stored content size", bytes(wrong_size)),
        ("block size above the maximum", bytes(too_large)),
        ("truncated skippable", struct.pack("<II", 0x184D2A50, 40) + b"short"),
    ]


REQUIRED_CLASSES = ["truncated header", "truncated block", "missing endmark", "flipped header checksum",
                    "reserved FLG bit", "block-size id 3", "flipped payload byte, block checksum",
                    "flipped payload byte, content checksum", "flipped content checksum",
                    "wrong stored content size", "block size above the maximum"]


def _single_outcome(f):
    try:
        return None, lz4.frame.decompress(f)
    except Exception as e:   # noqa: BLE001  (whatever the single call raises is the reference)
        return (type(e), str(e)), None


def test_errors_stay_local_and_match_the_single_call(gpu):
    bad = _corrupt_cases()
    assert set(REQUIRED_CLASSES) <= {name for name, _ in bad}
    good_in = [_distinct()[i] for i in (7, 6, 0, 15, 5, 22)]
    good = [lz4.frame.compress(d, content_checksum=bool(i & 1), block_checksum=bool(i & 2), block_linked=bool(i & 4))
            for i, d in enumerate(good_in)]
    frames, names = [], []
    for i, (name, f) in enumerate(bad):                       # g b g b ... : every bad frame between good ones
        frames += [good[i % len(good)], f]
        names += [None, name]
    frames.append(good[0])
    names.append(None)
    outcome = [_single_outcome(f) for f in frames]
    for name, (err, _res) in zip(names, outcome):
        assert (err is not None) == (name is not None), name   # every class is caught by the single call
    buf, off, ln = _pack(gpu, frames)
    out, o_off, o_len, status, read = lz4.frame.decompress_batch(buf, off, ln)
    st = status.cpu().tolist()
    outs = _cut(out, o_off, o_len)
    for i, (name, (err, res)) in enumerate(zip(names, outcome)):
        assert (st[i] != 0) == (err is not None), (i, name, st[i])
        if err is None:
            assert outs[i] == res, i
            assert read.cpu().tolist()[i] == len(frames[i])
    # the host form raises what the single call raises for the lowest failing index
    for start in range(1, len(frames), 2):
        want = outcome[start][0]
        with pytest.raises(want[0]) as e:
            lz4.frame.decompress_many(frames[start - 1:start + 4])
        assert str(e.value) == want[1], names[start]
    assert lz4.frame.decompress_many(good) == good_in


# ----------------------------------------------- lz4m_decompress_chains
def _chain_fixture(gpu):
    """Three chains of 1, 2 and 5 blocks (one stored) in one block table."""
    import torch
    t = _streams()["text"]
    rnd = _streams()["random"]
    plans = [[t[0:3000]],
             [t[1000:5000], t[3000:9000]],
             [t[0:2000], t[1000:4000], rnd[:1500], t[500:3500], t[100:70000][:40000]]]
    payloads, raw, first, count, want = [], [], [], [], []
    for blocks in plans:
        first.append(len(payloads))
        count.append(len(blocks))
        hist = b""
        for j, d in enumerate(blocks):
            stored = d is blocks[2] if len(blocks) == 5 else False
            payloads.append(d if stored else _blk(d, hist))
            raw.append(int(stored))
            hist += d
        want.append(hist)
    lens = [len(p) for p in payloads]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    src = torch.frombuffer(bytearray(b"".join(payloads)), dtype=torch.uint8).to(gpu)
    T = lambda v, dt: torch.tensor(np.asarray(v), dtype=dt, device=gpu)   # noqa: E731
    return (src, T(offs, torch.int64), T(lens, torch.int32), T(raw, torch.uint8), first, count, want, payloads)


def _run_chains(gpu, src, off, ln, raw, first, count, max_block=65536):
    """(bytes per chain, statuses) from lz4m_decompress_chains and from lz4m_decompress_chain run per chain."""
    import torch
    from lz4 import _native as N
    nb = off.numel()
    dst_off = np.concatenate([[0], np.cumsum([c * max_block for c in count])[:-1]]).astype(np.int64)
    total = int(sum(c * max_block for c in count)) + 64
    res = []
    for batched in (True, False):
        dst = torch.full((total,), 0xA5, dtype=torch.uint8, device=gpu)
        st = torch.full((nb,), -7, dtype=torch.int32, device=gpu)
        if batched:
            N.launch_decompress_chains(src, off, ln, raw, torch.tensor(first, dtype=torch.int64, device=gpu),
                                       torch.tensor(count, dtype=torch.int32, device=gpu), dst,
                                       torch.tensor(dst_off, dtype=torch.int64, device=gpu),
                                       torch.full((len(count),), max_block, dtype=torch.int32, device=gpu), st,
                                       len(count))
        else:
            for f, c, o in zip(first, count, dst_off):
                N.launch_decompress_chain(src, off[f:f + c], ln[f:f + c], raw[f:f + c] != 0, dst[int(o):],
                                          st[f:f + c], c, max_block)
        torch.cuda.synchronize()
        res.append((dst.cpu().numpy(), st.cpu().tolist(), dst_off))
    return res


def test_decompress_chains_equals_the_serial_chain(gpu):
    src, off, ln, raw, first, count, want, _ = _chain_fixture(gpu)
    (b_dst, b_st, dst_off), (s_dst, s_st, _) = _run_chains(gpu, src, off, ln, raw, first, count)
    assert b_st == s_st and min(b_st) > 0
    for c, w in enumerate(want):
        o = int(dst_off[c])
        assert b_dst[o:o + len(w)].tobytes() == w, c
        assert s_dst[o:o + len(w)].tobytes() == w, c
        assert sum(b_st[first[c]:first[c] + count[c]]) == len(w)
    assert b_dst[-64:].tobytes() == b"\xa5" * 64              # nothing past the last chain's capacity


def test_decompress_chains_failure_stays_in_its_chain(gpu):
    import torch
    src, off, ln, raw, first, count, want, payloads = _chain_fixture(gpu)
    bad = first[2] + 1                                         # the 5-block chain's second block
    src = src.clone()
    o, n = int(off[bad]), int(ln[bad])
    src[o:o + n] = 0xFF                                        # length bytes run past the block's end
    (b_dst, b_st, dst_off), (s_dst, s_st, _) = _run_chains(gpu, src, off, ln, raw, first, count)
    assert b_st == s_st
    assert b_st[bad] < 0 and b_st[bad + 1:bad + 4] == [-1, -1, -1] and b_st[first[2]] == 2000
    for c in (0, 1):                                           # the neighbours are intact
        o = int(dst_off[c])
        assert b_dst[o:o + len(want[c])].tobytes() == want[c]
        assert all(s > 0 for s in b_st[first[c]:first[c] + count[c]])
    # a chain of no blocks does nothing
    count0 = [count[0], 0, count[2]]
    (z_dst, z_st, z_off), _ = _run_chains(gpu, src, off, ln, raw, first, count0)
    assert z_st[first[1]:first[1] + count[1]] == [-7, -7]
    assert z_dst[int(z_off[0]):int(z_off[0]) + len(want[0])].tobytes() == want[0]


# ------------------------------------------------------------------ capacity
def test_results_are_packed_and_inside_their_buffers(gpu):
    """Neither call lets the caller pre-allocate, so the check is on the spans: in order, no overlap, no gap, the
    last one ending where the buffer ends -- no byte of the buffers belongs to no item -- and every item's bytes
    right (a write outside an item's span would land in a neighbour's)."""
    items = _mixed()[:64] + [b"", _distinct()[7], b""]
    buf, off, ln = _pack(gpu, items)
    for kw in (dict(), dict(block_linked=False, block_checksum=True, content_checksum=True, store_size=False)):
        frames, f_off, f_len = lz4.frame.compress_batch(buf, off, ln, **kw)
        _assert_back_to_back(frames, f_off, f_len)
        assert _cut(frames, f_off, f_len) == [_single(d, **kw) for d in items]
        out, o_off, o_len, status, read = lz4.frame.decompress_batch(frames, f_off, f_len)
        _assert_back_to_back(out, o_off, o_len)
        assert o_len.cpu().tolist() == [len(d) for d in items]
        assert _cut(out, o_off, o_len) == items
        assert status.cpu().tolist() == [0] * len(items)


def test_spans_outside_the_buffer_are_refused(gpu):
    import torch
    buf, off, ln = _pack(gpu, [b"abcdef" * 10])
    for o, n in ((0, 61), (-1, 4), (59, 2), (0, -1)):
        bo = torch.tensor([o], dtype=torch.int64, device=gpu)
        bn = torch.tensor([n], dtype=torch.int64, device=gpu)
        with pytest.raises(ValueError):
            lz4.frame.compress_batch(buf, bo, bn)
        with pytest.raises(ValueError):
            lz4.frame.decompress_batch(buf, bo, bn)
    e = torch.empty(0, dtype=torch.int64, device=gpu)
    assert [t.numel() for t in lz4.frame.compress_batch(buf, e, e)] == [0, 0, 0]
    assert [t.numel() for t in lz4.frame.decompress_batch(buf, e, e)] == [0, 0, 0, 0, 0]
    with pytest.raises(RuntimeError, match="ERROR_maxBlockSize_invalid"):
        lz4.frame.compress_batch(buf, off, ln, block_size=3)

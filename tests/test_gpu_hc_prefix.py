"""GPU tests of the HC compressor with a prefix (hc_prefix_kernel,
lz4m_compress_hc_dict_batch, compress_batch(dict_len=),
compress_many(mode="high_compression", dict=), lz4.frame.compress_device(
parse="hc")): its bytes equal the CPU model (hc_model_compress_prefix of
tests/hc_model/hc_model.c)
and decode on the device with the prefix as dictionary; an absent prefix gives
the old entry point's bytes; batches are independent of their layout; limited
output; C-ABI argument checks; dictionaries through compress_many; HC frames,
linked and independent; the kernels' resource report."""
import json
import os

import numpy as np
import pytest
import torch

import hc_prefix_support as HP
import hc_support as H
from conftest import GOLDEN

import lz4.block
import lz4.frame
from lz4 import _native as N, _synth

HC = "high_compression"
_outputs = H.outputs


class Batch:
    """Blocks in one host buffer, each with dict_len[i] and (where that is
    positive) its prefix immediately before it."""

    def __init__(self):
        self.chunks, self.size = [], 0
        self.off, self.len, self.dl = [], [], []

    def _append(self, data: bytes) -> int:
        at = self.size
        self.chunks.append(data)
        self.size += len(data)
        return at

    def add(self, prefix: bytes, block: bytes, dict_len: int | None = None):
        """block after prefix[-65536:]; dict_len defaults to len(prefix)"""
        at = self._append(prefix[-HP.PREFIX_MAX:] + block)
        self.off.append(at + min(len(prefix), HP.PREFIX_MAX))
        self.len.append(len(block))
        self.dl.append(len(prefix) if dict_len is None else dict_len)

    def add_cut(self, data: bytes, block: int):
        """data cut into blocks, each with the up to 64 KiB of data before it as its prefix"""
        at = self._append(data)
        for start in range(0, len(data), block):
            self.off.append(at + start)
            self.len.append(min(block, len(data) - start))
            self.dl.append(min(start, HP.PREFIX_MAX))

    def host(self) -> np.ndarray:
        return np.frombuffer(b"".join(self.chunks) + bytes(16), dtype=np.uint8)

    def prefix_len(self, i: int) -> int:
        return min(max(self.dl[i], 0), HP.PREFIX_MAX)

    def model(self, host: np.ndarray, i: int, level: int) -> bytes:
        return HP.model_compress_at(host, self.off[i], self.len[i], self.prefix_len(i), level)

    def device(self, dev):
        t = lambda v, dt: torch.tensor(v, dtype=dt, device=dev)   # noqa: E731
        return (torch.from_numpy(self.host().copy()).to(dev), t(self.off, torch.int64), t(self.len, torch.int32),
                t(self.dl, torch.int32))


def _assert_decodes(batch: Batch, src, off, ln, dst, dst_off, out_len):
    """Every block decodes on the device, its prefix as the dictionary, to its input."""
    assert bool((out_len > 0).all())
    P = torch.tensor([batch.prefix_len(i) for i in range(len(batch.off))], dtype=torch.int32, device=src.device)
    back, back_off, status = lz4.block.decompress_batch(dst, dst_off, out_len, ln, dict_buf=src,
                                                        dict_off=off - P.to(torch.int64), dict_len=P)
    assert torch.equal(status, ln)
    host, got, o = src.cpu().numpy(), back.cpu().numpy(), back_off.cpu().numpy()
    for i, (a, n) in enumerate(zip(batch.off, batch.len)):
        assert (got[int(o[i]):int(o[i]) + n] == host[a:a + n]).all(), f"block {i}"


@pytest.fixture(scope="module")
def equality_batch():
    b = Batch()
    for _, prefix, block in HP.grid_cases():
        b.add(prefix, block)
    for prefix, block in HP.edge_cases().values():
        b.add(prefix, block)
    text = _synth.word_text(np.random.default_rng(11), 65536 + 200003).tobytes()
    b.add(b"", text[:5000], dict_len=0)          # no prefix: the bytes before these two belong to other blocks
    b.add(b"", text[:5000], dict_len=-1)
    b.add(text[:30000], text[30000:65536])       # prefix + block = 65536: the last with position + 1 in the heads
    b.add(text[:30000], text[30000:65537])       # 65537: the first with rebased heads (the grid: to 131072, 131073)
    b.add(text[:65536], text[65536:])            # 200003 bytes after a full prefix: the chain index wraps
    b.add(bytes(100000) + text[:70000], text[1000:3000])   # a dictionary longer than 64 KiB: its tail counts
    b.add_cut(b"".join(H.kind_blocks("silesia")), 65536)
    return b


@pytest.mark.parametrize("level", [3, 4, 9, 12])
@pytest.mark.gpu
def test_kernel_bytes_equal_the_model(gpu, equality_batch, level):
    b = equality_batch
    src, off, ln, dl = b.device(gpu)
    dst, dst_off, out_len = lz4.block.compress_batch(src, off, ln, mode=HC, compression=level, dict_len=dl)
    _assert_decodes(b, src, off, ln, dst, dst_off, out_len)
    host = b.host()
    for i, got in enumerate(_outputs(dst, dst_off, out_len)):
        assert got == b.model(host, i, level), f"block {i} (prefix {b.dl[i]}, {b.len[i]} bytes) at level {level}"


@pytest.mark.gpu
def test_no_prefix_equals_the_old_entry_point(gpu):
    blocks = [d for _, d in H.validity_inputs() if len(d) <= 70000] + list(H.kind_blocks("silesia"))[:8]
    for value in (0, -1, -65536):
        b = Batch()
        for d in blocks:
            b.add(b"", d, dict_len=value)
        src, off, ln, dl = b.device(gpu)
        dst, dst_off, out_len = lz4.block.compress_batch(src, off, ln, mode=HC, compression=4, dict_len=dl)
        old = lz4.block.compress_batch(src, off, ln, mode=HC, compression=4)
        assert _outputs(dst, dst_off, out_len) == _outputs(*old), value


@pytest.fixture(scope="module")
def mixed_batch():
    """1024 blocks of 0..70000 bytes after prefixes of 0..65536 bytes, cut from the silesia mix (seeded)."""
    pool = _synth.blocks(64, "silesia", seed=78, block=140000)
    rng = np.random.default_rng(1024)
    lens = rng.integers(0, 70001, size=1024)
    pre = rng.integers(0, 65537, size=1024)
    lens[:4] = (0, 70000, 13, 12)
    pre[:6] = (65536, 65536, 5, 0, 0, 1)
    b = Batch()
    for i, (n, p) in enumerate(zip(lens, pre)):
        row = pool[i % 64]
        b.add(row[:int(p)].tobytes(), row[int(p):int(p) + int(n)].tobytes())
    return b


@pytest.mark.gpu
def test_batch_independence(gpu, mixed_batch):
    level, b = 4, mixed_batch
    src, off, ln, dl = b.device(gpu)
    cap = (ln.to(torch.int64) + ln.to(torch.int64) // 255 + 16).to(torch.int32)
    dst_off = N.exclusive_scan(cap)[:-1]
    total = int(cap.to(torch.int64).sum().item())
    runs = []
    for _ in range(2):
        dst = torch.zeros(total, dtype=torch.uint8, device=gpu)
        _, _, out_len = lz4.block.compress_batch(src, off, ln, dst=dst, dst_off=dst_off, dst_cap=cap, mode=HC,
                                                 compression=level, dict_len=dl)
        runs.append((dst, out_len))
    (dst, out_len), (dst2, out_len2) = runs
    assert torch.equal(out_len, out_len2) and torch.equal(dst, dst2)   # a second launch: the same bytes
    _assert_decodes(b, src, off, ln, dst, dst_off, out_len)
    outs = _outputs(dst, dst_off, out_len)
    host = b.host()
    for i in np.random.default_rng(32).choice(1024, size=32, replace=False):
        assert outs[i] == b.model(host, int(i), level), f"block {i}"
    for k in (0, 1, 2, 511, 1023):   # alone: the same bytes as inside the batch
        one = Batch()
        P = b.prefix_len(k)
        one.add(host[b.off[k] - P:b.off[k]].tobytes(), host[b.off[k]:b.off[k] + b.len[k]].tobytes())
        s1, o1, l1, d1 = one.device(gpu)
        assert _outputs(*lz4.block.compress_batch(s1, o1, l1, mode=HC, compression=level, dict_len=d1))[0] == outs[k]


@pytest.mark.gpu
def test_limited_output(gpu):
    level = 4
    b = Batch()
    for _, prefix, block in HP.grid_cases():
        if len(prefix) in (7, 4096, 65536) and len(block) <= 65536:
            b.add(prefix, block)
    for prefix, block in HP.edge_cases().values():
        b.add(prefix, block)
    b.add_cut(b"".join(H.kind_blocks("silesia")[:6]), 65536)
    src, off, ln, dl = b.device(gpu)
    dst, dst_off, out_len = lz4.block.compress_batch(src, off, ln, mode=HC, compression=level, dict_len=dl)
    full = _outputs(dst, dst_off, out_len)
    sizes = out_len.cpu().numpy().astype(np.int64)
    assert (sizes >= 1).all()
    guard = 64
    for caps in (sizes, sizes - 1):
        offs = np.zeros(len(sizes), dtype=np.int64)
        offs[1:] = np.cumsum(caps[:-1] + guard)
        total = int(offs[-1] + caps[-1] + guard)
        slot = np.zeros(total, dtype=bool)
        for o, c in zip(offs, caps):
            slot[o:o + c] = True
        d = torch.full((total,), 0xA5, dtype=torch.uint8, device=gpu)
        _, _, got = lz4.block.compress_batch(src, off, ln, dst=d, dst_off=torch.from_numpy(offs).to(gpu),
                                             dst_cap=torch.from_numpy(caps.astype(np.int32)).to(gpu), mode=HC,
                                             compression=level, dict_len=dl)
        host = d.cpu().numpy()
        assert (host[~slot] == 0xA5).all()   # the 64 bytes after every slot are intact
        if caps is sizes:
            assert (got.cpu().numpy() == sizes).all()   # an exact fit is accepted
            assert [host[o:o + c].tobytes() for o, c in zip(offs, caps)] == full
        else:
            assert (got.cpu().numpy() == 0).all()       # one byte short


@pytest.mark.gpu
def test_c_abi(gpu):
    lib = N.lib()
    fn = lib.lz4m_compress_hc_dict_batch
    assert fn(None, None, None, None, None, None, None, None, 0, 9, None, 0, None) == 0
    assert fn(None, None, None, None, None, None, None, None, -1, 9, None, 0, None) == N.EINVAL
    text = H.kind_blocks("text")
    b = Batch()
    for k, (prefix, block) in enumerate([(b"", b""), (b"y" * 7, b"x" * 100), (text[0], text[1]),
                                         (text[2][:999], text[3]), (bytes(65536), bytes(70000))]):
        b._append(bytes(1 + (b.size + min(len(prefix), 65536)) % 2))   # every block at an odd offset
        b.add(prefix, block)
    assert all(o % 2 == 1 for o in b.off)
    n = len(b.off)
    src, off, ln, dl = b.device(gpu)
    need = int(lib.lz4m_compress_hc_workspace_size(n, 70000))   # (compress_batch runs the larger one below)
    assert lib.lz4m_compress_hc_dict_workspace_size(n, 70000) == n * 262144 >= need
    assert lib.lz4m_compress_hc_dict_workspace_size(0, 70000) == 0
    assert lib.lz4m_compress_hc_dict_workspace_size(1 << 20, 65536) == 2560 * 262144
    cap = torch.tensor([H.compress_bound(k) for k in b.len], dtype=torch.int32, device=gpu)
    dst_off = N.exclusive_scan(cap)[:-1]
    dst = torch.zeros(int(cap.sum().item()), dtype=torch.uint8, device=gpu)
    out_len = torch.full((n,), -7, dtype=torch.int32, device=gpu)
    work = torch.empty(need + 2, dtype=torch.uint8, device=gpu)
    head = [N.ptr(src), N.ptr(off), N.ptr(ln)]
    tail = [N.ptr(dst), N.ptr(dst_off), N.ptr(cap), N.ptr(out_len), n, 9]
    sp = N.stream_ptr()
    assert fn(*head, N.ptr(dl), *tail, N.ptr(work), need - 1, sp) == N.EINVAL      # a short workspace
    assert fn(*head, N.ptr(dl), *tail, None, need, sp) == N.EINVAL                 # none
    assert fn(*head, N.ptr(dl), *tail, N.ptr(work) + 1, need, sp) == N.EINVAL      # an odd one
    assert fn(*head, None, *tail, N.ptr(work), need, sp) == N.EINVAL               # no dict_len
    torch.cuda.synchronize()
    assert (out_len.cpu().numpy() == -7).all()   # refused before any launch
    assert fn(*head, N.ptr(dl), *tail, N.ptr(work), need, sp) == 0
    host = b.host()
    for i, got in enumerate(_outputs(dst, dst_off, out_len)):
        assert got == b.model(host, i, 9), f"block {i}"


@pytest.mark.gpu
def test_compress_many_with_dict(gpu):
    text = _synth.word_text(np.random.default_rng(12), 70000 + 66000).tobytes()
    blocks = [text[70000:], b"", text[70000:71000], text[100:112], bytes(3000)]
    plain = lz4.block.compress_many(blocks, store_size=False, mode=HC, compression=4)
    for size in (0, 3, 1000, 70000):
        D = text[:size]
        for level in (4, 9):
            many = lz4.block.compress_many(blocks, store_size=False, mode=HC, compression=level, dict=D)
            assert many == [HP.model_compress_prefix(D, x, level) for x in blocks], (size, level)
            for x, comp in zip(blocks, many):
                assert lz4.block.decompress(comp, uncompressed_size=len(x), dict=D) == x
        if size == 0:
            assert lz4.block.compress_many(blocks, store_size=False, mode=HC, compression=4, dict=b"") == plain
    D = text[:70000]
    sized = lz4.block.compress_many(blocks[:1], mode=HC, compression=9, dict=D)[0]
    assert lz4.block.decompress(sized, dict=D) == blocks[0]
    assert len(sized) < len(lz4.block.compress_many(blocks[:1], mode=HC, compression=9)[0])   # the dictionary pays
    with pytest.raises(NotImplementedError, match="dict"):
        lz4.block.compress(blocks[0], mode=HC, dict=D)
    src = torch.zeros(64, dtype=torch.uint8, device=gpu)
    off = torch.zeros(1, dtype=torch.int64, device=gpu)
    ln = torch.full((1,), 32, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError, match="dict_len"):
        lz4.block.compress_batch(src, off, ln, mode="default", dict_len=torch.zeros(1, dtype=torch.int32, device=gpu))


# ------------------------------------------------------------------ frames
def _dev(b, gpu):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(gpu) if len(b) else \
        torch.empty(0, dtype=torch.uint8, device=gpu)


def _frame_payloads(frame: bytes, block_checksum: bool, content_size: bool = True):
    """[(raw, payload)] of a frame's blocks, and the position after the end mark."""
    pos = 7 + (8 if content_size else 0)
    out = []
    while True:
        word = int.from_bytes(frame[pos:pos + 4], "little")
        pos += 4
        if word == 0:
            return out, pos
        size = word & 0x7FFFFFFF
        out.append((bool(word >> 31), frame[pos:pos + size]))
        pos += size + (4 if block_checksum else 0)


@pytest.fixture(scope="module")
def frame_inputs():
    text = _synth.word_text(np.random.default_rng(13), 5 * 65536 + 1000).tobytes()
    rnd = np.random.default_rng(14).integers(0, 256, size=65536, dtype=np.uint8).tobytes()
    mix = _synth.blocks(13, "silesia", seed=15).tobytes()[:3 * 262144 + 7]
    return {
        "text-64k": (text, 4),
        "mix-256k": (mix, 5),
        "raw-middle": (text[:65536] + rnd + text[65536:65536 + 40100], 4),
        "one-block": (text[:65536], 4),
        "empty": (b"", 4),
    }


@pytest.mark.parametrize("checksums", [False, True])
@pytest.mark.parametrize("block_linked", [True, False])
@pytest.mark.parametrize("name", ["text-64k", "mix-256k", "raw-middle", "one-block", "empty"])
@pytest.mark.gpu
def test_hc_frames(gpu, frame_inputs, name, block_linked, checksums):
    import oracle as O
    data, bsid = frame_inputs[name]
    bsize = {4: 65536, 5: 262144}[bsid]
    linked = block_linked and len(data) > bsize
    ref = O.Reference() if os.path.exists(O.REF_SO) else None   # (the reference build, where it is present)
    d = _dev(data, gpu)
    for level in (3, 9):
        f = lz4.frame.compress_device(d, parse="hc", compression_level=level, block_size=bsid,
                                      block_linked=block_linked, content_checksum=checksums,
                                      block_checksum=checksums)
        frame = f.cpu().numpy().tobytes()
        info = lz4.frame.get_frame_info(frame)
        assert info["block_linked"] == linked and info["block_size"] == bsize
        assert info["content_checksum"] == checksums and info["block_checksum"] == checksums
        got, end = _frame_payloads(frame, checksums, content_size=len(data) > 0)   # (size 0 is not stored)
        assert end + (4 if checksums else 0) == len(frame)
        want = HP.linked_frame_parts(data, level, linked, block=bsize)
        assert [p for _, p in got] == want, (name, level)
        assert [raw for raw, _ in got] == [len(p) == min(bsize, len(data) - i * bsize) for i, p in enumerate(want)]
        if name == "raw-middle":
            assert [raw for raw, _ in got] == [False, True, False]
        assert lz4.frame.decompress_device(f).cpu().numpy().tobytes() == data
        assert lz4.frame.decompress(frame) == data
        if ref is not None:
            code, out = O.ref_decompress_frame(ref, frame)
            assert code == 0 and out == data
    if linked and name != "raw-middle":   # the history pays
        indep = lz4.frame.compress_device(d, parse="hc", compression_level=9, block_size=bsid, block_linked=False,
                                          content_checksum=checksums, block_checksum=checksums)
        assert len(frame) < indep.numel()


@pytest.mark.gpu
def test_frame_arguments_and_unchanged_paths(gpu):
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    arr = np.load(os.path.join(GOLDEN, "golden.npz"), allow_pickle=False)
    inputs = {e["name"]: arr[e["key"]].tobytes() for e in man["inputs"]}
    data = inputs["text_300k"]
    d = _dev(data, gpu)
    with pytest.raises(ValueError, match="compression_level"):
        lz4.frame.compress_device(d, parse="hc", compression_level=2)
    with pytest.raises(ValueError, match="compression_level"):
        lz4.frame.compress_device(d, parse="hc")
    with pytest.raises(ValueError, match="parse"):
        lz4.frame.compress_device(d, parse="optimal", compression_level=9)
    with pytest.raises(NotImplementedError):
        lz4.frame.compress_device(d, compression_level=3)
    with pytest.raises(NotImplementedError):
        lz4.frame.compress_device(d, compression_level=3, parse="parallel")
    with pytest.raises(NotImplementedError):
        lz4.frame.compress(data, compression_level=3)
    # parse="exact" still gives the reference's frames (golden vectors: linked and independent 64 KiB blocks)
    for e in man["frames"]:
        o = e["opts"]
        if e["input"] != "text_300k" or o["block_size_id"] != 4 or o.get("level", 0) != 0:
            continue
        f = lz4.frame.compress_device(d, parse="exact", block_size=4, block_linked=o["linked"],
                                      content_checksum=o.get("content_checksum", False),
                                      block_checksum=o.get("block_checksum", False))
        assert f.cpu().numpy().tobytes() == arr[e["key"]].tobytes(), o
    # parse="parallel" is its own parse: a valid frame of the input, twice the same bytes
    p1 = lz4.frame.compress_device(d, parse="parallel", block_size=4, block_linked=False)
    p2 = lz4.frame.compress_device(d, parse="parallel", block_size=4, block_linked=False)
    assert torch.equal(p1, p2) and lz4.frame.decompress(p1.cpu().numpy().tobytes()) == data


def test_hc_prefix_kernels_use_no_scratch():
    """The compiler's resource report of lz4m_hc.hip (kept by the csrc Makefile): the
    three hc_prefix_kernel instances use 0 bytes of scratch."""
    seen = 0
    for name, scratch in H.scratch_report("lz4m_hc.res"):
        if "hc_prefix_kernel" in name:
            assert scratch == 0, f"{name} uses {scratch} B/lane of scratch"
            seen += 1
    assert seen == 3   # prefix + block up to 64 KiB, up to 128 KiB, and beyond

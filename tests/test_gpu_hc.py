"""GPU tests of the hash-chain (HC) block compressor (lz4m_hc.hip,
lz4m_compress_hc_batch, lz4.block.compress(mode="high_compression")): its
bytes equal the CPU model of the parse (tests/hc_model/hc_model.c) and decode
on the device; batches are independent of their layout; limited output;
C-ABI argument checks; the drop-in API; the kernel's resource report."""
import json
import os

import numpy as np
import pytest
import torch

import hc_support as H
from conftest import GOLDEN

import lz4.block
from lz4 import _native as N

HC = "high_compression"
_pack, _outputs, _assert_decodes = H.pack, H.outputs, H.assert_decodes


def _compress(blocks, dev, level, **kw):
    src, off, ln = _pack(blocks, dev)
    dst, dst_off, out_len = lz4.block.compress_batch(src, off, ln, mode=HC, compression=level, **kw)
    return src, off, ln, dst, dst_off, out_len


@pytest.fixture(scope="module")
def equality_inputs():
    blocks = [d for _, d in H.validity_inputs()] + [d for _, d in H.window_inputs()]
    for kind in H.KINDS:
        blocks += list(H.kind_blocks(kind))
    return blocks


@pytest.mark.parametrize("level", [3, 4, 7, 9, 12])
@pytest.mark.gpu
def test_kernel_bytes_equal_the_model(gpu, equality_inputs, level):
    src, off, ln, dst, dst_off, out_len = _compress(equality_inputs, gpu, level)
    _assert_decodes(src, ln, dst, dst_off, out_len)
    for i, (data, got) in enumerate(zip(equality_inputs, _outputs(dst, dst_off, out_len))):
        assert got == H.model_compress(data, level), f"block {i} ({len(data)} bytes) at level {level}"


@pytest.fixture(scope="module")
def mixed_batch():
    return H.mixed_batch()


@pytest.mark.gpu
def test_batch_independence(gpu, mixed_batch):
    level = 4
    src, off, ln = _pack(mixed_batch, gpu)
    cap = (ln.to(torch.int64) + ln.to(torch.int64) // 255 + 16).to(torch.int32)
    dst_off = N.exclusive_scan(cap)[:-1]
    total = int(cap.to(torch.int64).sum().item())
    runs = []
    for _ in range(2):
        dst = torch.zeros(total, dtype=torch.uint8, device=gpu)
        _, _, out_len = lz4.block.compress_batch(src, off, ln, dst=dst, dst_off=dst_off, dst_cap=cap, mode=HC,
                                                 compression=level)
        runs.append((dst, out_len))
    (dst, out_len), (dst2, out_len2) = runs
    assert torch.equal(out_len, out_len2) and torch.equal(dst, dst2)   # a second launch: the same bytes
    _assert_decodes(src, ln, dst, dst_off, out_len)
    outs = _outputs(dst, dst_off, out_len)
    for i in np.random.default_rng(64).choice(4096, size=64, replace=False):
        assert outs[i] == H.model_compress(mixed_batch[i], level), f"block {i}"
    for k in (0, 1, 2047, 4095):   # alone: the same bytes as inside the batch
        _, _, _, d1, o1, n1 = _compress([mixed_batch[k]], gpu, level)
        assert _outputs(d1, o1, n1)[0] == outs[k], f"block {k}"


@pytest.mark.gpu
def test_limited_output(gpu):
    level = 4
    blocks = [d for _, d in H.validity_inputs() if len(d) <= 70000] + list(H.kind_blocks("silesia"))[:8]
    src, off, ln, dst, dst_off, out_len = _compress(blocks, gpu, level)
    full = _outputs(dst, dst_off, out_len)
    sizes = out_len.cpu().numpy().astype(np.int64)
    assert (sizes >= 1).all()
    guard = 64
    for caps in (sizes, sizes - 1, np.zeros_like(sizes)):
        offs = np.zeros(len(blocks), dtype=np.int64)
        offs[1:] = np.cumsum(caps[:-1] + guard)
        total = int(offs[-1] + caps[-1] + guard)
        slot = np.zeros(total, dtype=bool)
        for o, c in zip(offs, caps):
            slot[o:o + c] = True
        d = torch.full((total,), 0xA5, dtype=torch.uint8, device=gpu)
        _, _, got = lz4.block.compress_batch(src, off, ln, dst=d, dst_off=torch.from_numpy(offs).to(gpu),
                                             dst_cap=torch.from_numpy(caps.astype(np.int32)).to(gpu), mode=HC,
                                             compression=level)
        host = d.cpu().numpy()
        assert (host[~slot] == 0xA5).all()   # the 64 bytes after every slot are intact
        if caps is sizes:
            assert (got.cpu().numpy() == sizes).all()
            assert [host[o:o + c].tobytes() for o, c in zip(offs, caps)] == full
        else:
            assert (got.cpu().numpy() == 0).all()


@pytest.mark.gpu
def test_c_abi(gpu):
    lib = N.lib()
    blocks = [b"", b"x" * 100] + list(H.kind_blocks("text"))[:3] + [bytes(70000)]
    n = len(blocks)
    assert lib.lz4m_compress_hc_batch(None, None, None, None, None, None, None, 0, 9, None, 0, None) == 0
    assert lib.lz4m_compress_hc_batch(None, None, None, None, None, None, None, -1, 9, None, 0, None) == N.EINVAL
    need = int(lib.lz4m_compress_hc_workspace_size(n, 70000))
    assert need >= n * 65536 * 2 and lib.lz4m_compress_hc_workspace_size(0, 70000) == 0
    assert lib.lz4m_compress_hc_workspace_size(1 << 20, 65536) <= 2560 * 65536 * 2
    # odd source offsets (no alignment is assumed)
    src, off, ln = _pack(blocks, gpu, first=1, gap=1)
    off = off + (off % 2 == 0).to(torch.int64)
    host = src.cpu().numpy()
    placed = [host[int(o):int(o) + len(b)].tobytes() for o, b in zip(off.cpu().numpy(), blocks)]
    cap = torch.tensor([H.compress_bound(len(b)) for b in blocks], dtype=torch.int32, device=gpu)
    dst_off = N.exclusive_scan(cap)[:-1]
    dst = torch.zeros(int(cap.sum().item()), dtype=torch.uint8, device=gpu)
    out_len = torch.full((n,), -7, dtype=torch.int32, device=gpu)
    work = torch.empty(need, dtype=torch.uint8, device=gpu)
    args = [N.ptr(src), N.ptr(off), N.ptr(ln), N.ptr(dst), N.ptr(dst_off), N.ptr(cap), N.ptr(out_len), n, 9]
    sp = N.stream_ptr()
    assert lib.lz4m_compress_hc_batch(*args, N.ptr(work), need - 1, sp) == N.EINVAL
    assert lib.lz4m_compress_hc_batch(*args, None, need, sp) == N.EINVAL
    torch.cuda.synchronize()
    assert (out_len.cpu().numpy() == -7).all()   # refused before any launch
    assert lib.lz4m_compress_hc_batch(*args, N.ptr(work), need, sp) == 0
    for data, got in zip(placed, _outputs(dst, dst_off, out_len)):
        assert got == H.model_compress(data, 9)


@pytest.mark.gpu
def test_block_api(gpu):
    x = H.kind_blocks("source")[0] + b"tail" * 5
    for c in (-1, 0, 3, 9, 12, 100):
        for store_size in (True, False):
            comp = lz4.block.compress(x, mode=HC, compression=c, store_size=store_size)
            assert isinstance(comp, bytes) and len(comp) < len(x) // 2
            back = lz4.block.decompress(comp) if store_size else lz4.block.decompress(comp, uncompressed_size=len(x))
            assert back == x
        assert lz4.block.compress(x, mode=HC, compression=c, store_size=False) == H.model_compress(x, c)
    ba = lz4.block.compress(x, mode=HC, compression=9, return_bytearray=True)
    assert isinstance(ba, bytearray) and lz4.block.decompress(ba) == x
    assert lz4.block.compress(b"", mode=HC, store_size=False) == b"\x00"
    with pytest.raises(OverflowError):
        lz4.block.compress(x, mode=HC, compression=2**31)
    with pytest.raises(NotImplementedError, match="dict"):
        lz4.block.compress(x, mode=HC, dict=b"abc" * 10)
    many = lz4.block.compress_many([x, b"", x[:1000]], store_size=False, mode=HC, compression=4)
    assert many == [H.model_compress(b, 4) for b in (x, b"", x[:1000])]


@pytest.mark.gpu
def test_default_mode_is_unchanged(gpu):
    """mode='default' still gives the reference's lz4.block.compress bytes (one golden block)."""
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    arr = np.load(os.path.join(GOLDEN, "golden.npz"), allow_pickle=False)
    inputs = {e["name"]: arr[e["key"]].tobytes() for e in man["inputs"]}
    e = next(e for e in man["compress"] if e["mode"] == "block_api" and e["accel"] == 1)
    want = arr[e["key"]].tobytes()
    data = inputs[e["input"]]
    assert lz4.block.compress(data, mode="default", store_size=False) == want
    assert lz4.block.compress_many([data], store_size=False) == [want]
    src, off, ln = _pack([data], gpu)
    dst, dst_off, out_len = lz4.block.compress_batch(src, off, ln)
    assert _outputs(dst, dst_off, out_len) == [want]


def test_hc_kernel_uses_no_scratch():
    """The compiler's resource report of lz4m_hc.hip (kept by the csrc Makefile): 0 bytes of scratch."""
    seen = 0
    for name, scratch in H.scratch_report("lz4m_hc.res"):
        if "hc_compress_kernel" in name:
            assert scratch == 0, f"{name} uses {scratch} B/lane of scratch"
            seen += 1
    assert seen == 2   # the <= 64 KiB kernel and the long-block kernel

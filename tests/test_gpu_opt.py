"""GPU tests of the optimal-parse block compressor (lz4m_opt.hip,
lz4m_compress_opt_batch, lz4.block.compress(mode="optimal")): its bytes equal
the CPU model of the parse (tests/hc_model/opt_model.c) and decode on the
device; batches are independent of their layout and of the workspace's
contents; limited output; slot containment under a scattered layout; C-ABI
argument checks; the block and frame APIs; the kernels' resource report."""

import numpy as np
import pytest
import torch

import hc_support as H
import layout_support as LS
import opt_support as P
import lz4.block
import lz4.frame
from lz4 import _native as N

OPT = "optimal"
_pack, _outputs, _assert_decodes = H.pack, H.outputs, H.assert_decodes


def _compress(blocks, dev, level, **kw):
    src, off, ln = _pack(blocks, dev)
    dst, dst_off, out_len = lz4.block.compress_batch(src, off, ln, mode=OPT, compression=level, **kw)
    return src, off, ln, dst, dst_off, out_len


def _launch(lib, src, off, ln, dst, dst_off, cap, out_len, level, work):
    return lib.lz4m_compress_opt_batch(N.ptr(src), N.ptr(off), N.ptr(ln), N.ptr(dst), N.ptr(dst_off), N.ptr(cap),
                                       N.ptr(out_len), off.numel(), level, N.ptr(work), work.numel(),
                                       N.stream_ptr())


@pytest.fixture(scope="module")
def equality_inputs():
    blocks = [d for _, d in H.validity_inputs()] + [d for _, d in H.window_inputs()]
    for kind in H.KINDS:
        blocks += list(H.kind_blocks(kind))
    return blocks


@pytest.mark.parametrize("level", [3, 4, 9])
@pytest.mark.gpu
def test_kernel_bytes_equal_the_model(gpu, equality_inputs, level):
    src, off, ln, dst, dst_off, out_len = _compress(equality_inputs, gpu, level)
    _assert_decodes(src, ln, dst, dst_off, out_len)
    for i, (data, got) in enumerate(zip(equality_inputs, _outputs(dst, dst_off, out_len))):
        assert got == P.model_compress(data, level), f"block {i} ({len(data)} bytes) at level {level}"


@pytest.fixture(scope="module")
def mixed_batch():
    return H.mixed_batch()


@pytest.mark.gpu
def test_batch_independence(gpu, mixed_batch):
    """Two launches on a workspace pre-filled with 0xFF: the same bytes, the
    model's, and those of each block compressed alone."""
    level = 4
    lib = N.lib()
    src, off, ln = _pack(mixed_batch, gpu)
    cap = (ln.to(torch.int64) + ln.to(torch.int64) // 255 + 16).to(torch.int32)
    dst_off = N.exclusive_scan(cap)[:-1]
    total = int(cap.to(torch.int64).sum().item())
    need = int(lib.lz4m_compress_opt_workspace_size(len(mixed_batch), 70000))
    runs = []
    for _ in range(2):
        work = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu)
        dst = torch.zeros(total, dtype=torch.uint8, device=gpu)
        out_len = torch.full((len(mixed_batch),), -7, dtype=torch.int32, device=gpu)
        assert _launch(lib, src, off, ln, dst, dst_off, cap, out_len, level, work) == 0
        runs.append((dst, out_len))
        del work
    (dst, out_len), (dst2, out_len2) = runs
    assert torch.equal(out_len, out_len2) and torch.equal(dst, dst2)
    _assert_decodes(src, ln, dst, dst_off, out_len)
    outs = _outputs(dst, dst_off, out_len)
    for i in np.random.default_rng(64).choice(4096, size=64, replace=False):
        assert outs[i] == P.model_compress(mixed_batch[i], level), f"block {i}"
    for k in (0, 1, 2047, 4095):   # alone: the same bytes as inside the batch
        _, _, _, d1, o1, n1 = _compress([mixed_batch[k]], gpu, level)
        assert _outputs(d1, o1, n1)[0] == outs[k], f"block {k}"


@pytest.fixture(scope="module")
def limited_blocks():
    return [d for _, d in H.validity_inputs() if len(d) <= 70000] + list(H.kind_blocks("silesia"))[:8]


@pytest.mark.gpu
def test_limited_output(gpu, limited_blocks):
    level = 4
    blocks = limited_blocks
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
                                             dst_cap=torch.from_numpy(caps.astype(np.int32)).to(gpu), mode=OPT,
                                             compression=level)
        host = d.cpu().numpy()
        assert (host[~slot] == 0xA5).all()   # nothing outside a slot changed
        if caps is sizes:
            assert (got.cpu().numpy() == sizes).all()
            assert [host[o:o + c].tobytes() for o, c in zip(offs, caps)] == full
        else:
            assert (got.cpu().numpy() == 0).all()
            assert (host == 0xA5).all()      # a block that does not fit writes nothing


@pytest.mark.parametrize("cap_kind", ["bound", "exact", "short"])
@pytest.mark.gpu
def test_stays_in_its_slots_under_a_scattered_layout(gpu, limited_blocks, cap_kind):
    """Slots in a random order between poisoned gaps, sources in another order
    between 0xFF bytes, both bases off their allocations' alignment."""
    level, poison, seed = 3, 0xA5, 950
    blocks = limited_blocks
    sizes = [len(P.model_compress(b, level)) for b in blocks]
    caps = {"bound": [H.compress_bound(len(b)) for b in blocks], "exact": sizes,
            "short": [max(s - 1 - i % 3, 0) for i, s in enumerate(sizes)]}[cap_kind]
    dst_off, total = LS.plan_slots(caps, seed, first=13)
    alloc, src_off = LS.plan_sources(blocks, seed)
    src = torch.from_numpy(alloc).to(gpu)[1:]
    dst = torch.full((total,), poison, dtype=torch.uint8, device=gpu)
    ln = torch.tensor([len(b) for b in blocks], dtype=torch.int32, device=gpu)
    _, _, out_len = lz4.block.compress_batch(src, torch.from_numpy(src_off).to(gpu), ln, dst=dst,
                                             dst_off=torch.from_numpy(dst_off).to(gpu),
                                             dst_cap=torch.tensor(caps, dtype=torch.int32, device=gpu), mode=OPT,
                                             compression=level)
    host = dst.cpu().numpy()
    LS.assert_outside_intact(host, dst_off, caps, poison, cap_kind)
    got = out_len.cpu().numpy()
    for i, b in enumerate(blocks):
        if cap_kind == "short":
            assert got[i] == 0, i
        else:
            assert host[dst_off[i]:dst_off[i] + got[i]].tobytes() == P.model_compress(b, level), i


@pytest.mark.gpu
def test_c_abi(gpu):
    lib = N.lib()
    blocks = [b"", b"x" * 100] + list(H.kind_blocks("text"))[:3] + [bytes(70000)]
    n = len(blocks)
    assert lib.lz4m_compress_opt_batch(None, None, None, None, None, None, None, 0, 9, None, 0, None) == 0
    assert lib.lz4m_compress_opt_batch(None, None, None, None, None, None, None, -1, 9, None, 0, None) == N.EINVAL
    need = int(lib.lz4m_compress_opt_workspace_size(n, 70000))
    assert need >= n * 70000 * 10 and lib.lz4m_compress_opt_workspace_size(0, 70000) == 0
    # bounded whatever the number of blocks: 10 bytes per position for 2560 wavefronts
    assert lib.lz4m_compress_opt_workspace_size(1 << 20, 65536) == 2560 * (65536 + 64) * 10
    floor = int(lib.lz4m_compress_opt_workspace_size(n, 0))
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
    assert lib.lz4m_compress_opt_batch(*args, N.ptr(work), floor - 1, sp) == N.EINVAL
    assert lib.lz4m_compress_opt_batch(*args, None, need, sp) == N.EINVAL
    assert lib.lz4m_compress_opt_batch(*args, N.ptr(work) + 1, need - 1, sp) == N.EINVAL
    torch.cuda.synchronize()
    assert (out_len.cpu().numpy() == -7).all()   # refused before any launch
    assert lib.lz4m_compress_opt_batch(*args, N.ptr(work), need, sp) == 0
    for data, got in zip(placed, _outputs(dst, dst_off, out_len)):
        assert got == P.model_compress(data, 9)
    # a workspace sized for shorter blocks: the longer ones report 0, the others their bytes
    small = int(lib.lz4m_compress_opt_workspace_size(n, 100))
    assert lib.lz4m_compress_opt_batch(*args, N.ptr(work), small, sp) == 0
    got = out_len.cpu().numpy()
    assert [int(g) for g in got] == [1, len(P.model_compress(placed[1], 9)), 0, 0, 0, 0]


@pytest.mark.gpu
def test_block_api(gpu):
    x = H.kind_blocks("source")[0] + b"tail" * 5
    for c in (-1, 0, 3, 9, 12, 100):
        for store_size in (True, False):
            comp = lz4.block.compress(x, mode=OPT, compression=c, store_size=store_size)
            assert isinstance(comp, bytes) and len(comp) < len(x) // 2
            back = lz4.block.decompress(comp) if store_size else lz4.block.decompress(comp, uncompressed_size=len(x))
            assert back == x
        assert lz4.block.compress(x, mode=OPT, compression=c, store_size=False) == P.model_compress(x, c)
    ba = lz4.block.compress(x, mode=OPT, compression=9, return_bytearray=True)
    assert isinstance(ba, bytearray) and lz4.block.decompress(ba) == x
    assert lz4.block.compress(b"", mode=OPT, store_size=False) == b"\x00"
    with pytest.raises(NotImplementedError, match="dict"):
        lz4.block.compress(x, mode=OPT, dict=b"abc" * 10)
    with pytest.raises(NotImplementedError, match="dict"):
        lz4.block.compress_many([x], mode=OPT, dict=b"abc" * 10)
    with pytest.raises(NotImplementedError, match="dict"):
        src, off, ln = _pack([x], gpu)
        lz4.block.compress_batch(src, off, ln, mode=OPT, dict_len=torch.zeros(1, dtype=torch.int32, device=gpu))
    many = lz4.block.compress_many([x, b"", x[:1000]], store_size=False, mode=OPT, compression=4)
    assert many == [P.model_compress(b, 4) for b in (x, b"", x[:1000])]


@pytest.mark.gpu
def test_high_compression_level_12_is_unchanged(gpu):
    x = H.kind_blocks("source")[0] + b"tail" * 5
    got = lz4.block.compress(x, mode="high_compression", compression=12, store_size=False)
    assert got == H.model_compress(x, 12)
    assert got != P.model_compress(x, 12)


def _frame_payloads(frame: bytes, nblocks: int):
    """The block payloads of a frame without checksums whose header stores the content size."""
    pos, out = 15, []
    for _ in range(nblocks):
        word = int.from_bytes(frame[pos:pos + 4], "little")
        size = word & 0x7FFFFFFF
        out.append((bool(word >> 31), frame[pos + 4:pos + 4 + size]))
        pos += 4 + size
    assert frame[pos:pos + 4] == b"\x00\x00\x00\x00" and pos + 4 == len(frame)
    return out


@pytest.mark.gpu
def test_frame_api(gpu):
    data = b"".join(H.kind_blocks("text")[:3]) + H.kind_blocks("source")[0][:1000]
    assert len(data) == 3 * 65536 + 1000
    d_src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(gpu)
    frame = lz4.frame.compress_device(d_src, parse=OPT, compression_level=9, block_linked=False)
    back = lz4.frame.decompress_device(frame)
    assert back.cpu().numpy().tobytes() == data
    pieces = [data[i:i + 65536] for i in range(0, len(data), 65536)]
    for piece, (raw, payload) in zip(pieces, _frame_payloads(frame.cpu().numpy().tobytes(), 4)):
        assert not raw and payload == P.model_compress(piece, 9)
    with pytest.raises(NotImplementedError, match="linked"):
        lz4.frame.compress_device(d_src, parse=OPT, compression_level=9, block_linked=True)
    off = torch.tensor([0, 65536], dtype=torch.int64, device=gpu)
    ln = torch.tensor([65536, len(data) - 65536], dtype=torch.int64, device=gpu)
    frames, f_off, f_len = lz4.frame.compress_batch(d_src, off, ln, parse=OPT, compression_level=9,
                                                    block_linked=False)
    host = frames.cpu().numpy().tobytes()
    for o, k, lo, hi in zip(f_off.tolist(), f_len.tolist(), (0, 65536), (65536, len(data))):
        one = lz4.frame.compress_device(d_src[lo:hi].contiguous(), parse=OPT, compression_level=9,
                                        block_linked=False)
        assert host[o:o + k] == one.cpu().numpy().tobytes()
    with pytest.raises(NotImplementedError, match="linked"):
        lz4.frame.compress_batch(d_src, off, ln, parse=OPT, compression_level=9)


def test_opt_kernels_use_no_scratch():
    """The compiler's resource report of lz4m_opt.hip (kept by the csrc Makefile): 0 bytes of scratch."""
    seen = 0
    for name, scratch in H.scratch_report("lz4m_opt.res"):
        assert "hc_compress_kernel" not in name
        assert scratch == 0, f"{name} uses {scratch} B/lane of scratch"
        seen += 1
    assert seen == 2   # the <= 64 KiB kernel and the long-block kernel

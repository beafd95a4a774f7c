"""Argument handling of the parallel parse with a shared dictionary that needs
no device: the C entry points' checks, the Python keyword's, and the
dictionary kernel's resources."""
import pytest


def test_c_entry_points_validate_without_gpu():
    """LZ4M_EINVAL before any HIP call; n == 0 is a no-op."""
    import ctypes as C
    from lz4 import _native as N
    lib = N.lib()
    assert lib.lz4m_pcompress_dict_table_bytes() == 8192
    buf = (C.c_uint8 * (8192 + 64))()
    a = C.addressof(buf)
    tab = (a + 15) & ~15          # an aligned stand-in for a table (never dereferenced: every call fails first)
    dic = a + 8192
    # prepare: negative length, short table, null table, misaligned table, null dictionary with a length
    assert lib.lz4m_pcompress_dict_prepare(dic, -1, tab, 8192, None) == N.EINVAL
    assert lib.lz4m_pcompress_dict_prepare(dic, 16, tab, 8191, None) == N.EINVAL
    assert lib.lz4m_pcompress_dict_prepare(dic, 16, tab, 0, None) == N.EINVAL
    assert lib.lz4m_pcompress_dict_prepare(dic, 16, None, 8192, None) == N.EINVAL
    assert lib.lz4m_pcompress_dict_prepare(dic, 16, tab + 4, 8192, None) == N.EINVAL
    assert lib.lz4m_pcompress_dict_prepare(None, 16, tab, 8192, None) == N.EINVAL
    # batch: n < 0, dict_len < 0, null table or dictionary with dict_len > 0
    args = (None, None, None, None)   # d_dst, d_dst_off, d_dst_cap, d_out_len
    assert lib.lz4m_pcompress_dict_batch(None, None, None, dic, 16, tab, *args, -1, None) == N.EINVAL
    assert lib.lz4m_pcompress_dict_batch(None, None, None, dic, -1, tab, *args, 4, None) == N.EINVAL
    assert lib.lz4m_pcompress_dict_batch(None, None, None, dic, 16, None, *args, 4, None) == N.EINVAL
    assert lib.lz4m_pcompress_dict_batch(None, None, None, None, 16, tab, *args, 4, None) == N.EINVAL
    assert lib.lz4m_pcompress_dict_batch(None, None, None, dic, 16, tab + 4, *args, 4, None) == N.EINVAL
    # n == 0: nothing to do, with or without a dictionary
    assert lib.lz4m_pcompress_dict_batch(None, None, None, dic, 16, tab, *args, 0, None) == 0
    assert lib.lz4m_pcompress_dict_batch(None, None, None, None, 0, None, *args, 0, None) == 0


def test_compress_batch_rejects_dict_buf_combinations_without_gpu():
    """Raised before any device use (these tensors are host tensors)."""
    import torch
    import lz4.block
    from lz4 import _native as N
    src = torch.zeros(16, dtype=torch.uint8)
    off = torch.zeros(1, dtype=torch.int64)
    ln = torch.full((1,), 16, dtype=torch.int32)
    d = torch.zeros(64, dtype=torch.uint8)
    for table in ("block", "default", N.TABLE_U16_HASH4, N.PARSE_PARALLEL_HQ, N.PARSE_PARALLEL_LARGE):
        with pytest.raises(ValueError, match="PARSE_PARALLEL"):
            lz4.block.compress_batch(src, off, ln, table=table, dict_buf=d)
    with pytest.raises(ValueError, match="PARSE_PARALLEL"):
        lz4.block.compress_batch(src, off, ln, dict_buf=d)   # the default table
    with pytest.raises(ValueError, match="high_compression"):
        lz4.block.compress_batch(src, off, ln, table=N.PARSE_PARALLEL, mode="high_compression", dict_buf=d)
    with pytest.raises(ValueError, match="dict_len"):
        lz4.block.compress_batch(src, off, ln, table=N.PARSE_PARALLEL, dict_buf=d,
                                 dict_len=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="dict_len"):
        lz4.block.compress_batch(src, off, ln, table=N.PARSE_PARALLEL, mode="high_compression", dict_buf=d,
                                 dict_len=torch.zeros(1, dtype=torch.int32))
    assert lz4.block.PreparedDict.__slots__ == ("tail", "dict_len", "table")


def test_dictionary_kernel_keeps_its_occupancy():
    """The DICT instantiation of pcompress_kernel stays at 5 waves per SIMD
    without scratch (it holds there only because what derives from the lane id
    is rematerialised; a compiler that stops doing so
    would spill, or drop a wave, silently).  From the resource report the csrc
    Makefile keeps next to the object."""
    import os
    import re
    import subprocess
    from conftest import ROOT
    csrc = os.path.join(ROOT, "python-lz4_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc], check=True, capture_output=True)
    text = open(os.path.join(csrc, "build", "lz4m_pcompress.res")).read()
    # pcompress_kernel<false, 12, false, false, true>
    parts = re.split(r"Function Name: (\S+)", text)
    found = {parts[i]: parts[i + 1] for i in range(1, len(parts) - 1, 2)}
    dict_kernels = [k for k in found if "pcompress_kernelILb0ELi12ELb0ELb0ELb1E" in k]
    assert len(dict_kernels) == 1, sorted(found)

    def field(name):
        return int(re.search(re.escape(name) + r": (\d+)", found[dict_kernels[0]]).group(1))

    assert field("ScratchSize [bytes/lane]") == 0
    assert field("Occupancy [waves/SIMD]") == 5
    assert field("VGPRs") <= 96
    assert field("LDS Size [bytes/block]") == 8192

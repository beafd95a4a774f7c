"""CPU tests of the decoded-size pass's boundary: the C-ABI declares and
exports lz4m_decompressed_size_batch, its argument checks need no GPU, and
lz4.block's new forms check their arguments before they look for a device."""
import pytest

from test_capi import declared_symbols


def test_header_declares_and_library_exports_the_size_pass():
    from lz4 import _native as N
    assert "lz4m_decompressed_size_batch" in declared_symbols()
    assert hasattr(N.lib(), "lz4m_decompressed_size_batch")
    txt = open(__import__("test_capi").HEADER).read()
    for name in ("LZ4M_SIZE_OVERFLOW", "LZ4M_WALK_AUTO", "LZ4M_WALK_LANE", "LZ4M_WALK_WAVE"):
        assert f"#define {name}" in txt, name
    assert N.WALKS == {"auto": 0, "lane": 1, "wave": 2} and N.SIZE_OVERFLOW == -(2**31)


def test_argument_validation_without_gpu():
    """n == 0 is a no-op; n < 0 and an unknown walk are rejected before any HIP call."""
    from lz4 import _native as N
    f = N.lib().lz4m_decompressed_size_batch
    for walk in N.WALKS.values():
        assert f(None, None, None, None, None, 0, walk, None) == 0
        assert f(None, None, None, None, None, -1, walk, None) == N.EINVAL
    for walk in (7, 3, -1):
        assert f(None, None, None, None, None, 0, walk, None) == N.EINVAL
        assert f(None, None, None, None, None, 4, walk, None) == N.EINVAL
    with pytest.raises(ValueError, match="walk"):
        N.launch_decompressed_size(None, None, None, None, 0, walk="row")


def test_unknown_size_reaches_the_device_check():
    """uncompressed_size=None is an accepted argument: without a device the
    call gets as far as the "no HIP device" error, not a TypeError."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import lz4.block
    with pytest.raises(RuntimeError, match="no HIP device"):
        lz4.block.decompress_many([b"x"], uncompressed_size=None)
    with pytest.raises(RuntimeError, match="no HIP device"):
        lz4.block.decompress_many([b"x", b"\x01\x00\x00\x00\x10y"], uncompressed_size=[None, -1])
    with pytest.raises(RuntimeError, match="no HIP device"):
        lz4.block.decompressed_size_many([b"x"])
    with pytest.raises(TypeError):
        lz4.block.decompress_many(["x"], uncompressed_size=None)   # the argument checks still come first

"""CPU tests of the batched frame calls (lz4.frame.compress_many /
decompress_many / compress_batch / decompress_batch): what they answer
without a device, and that the C-ABI entry points behind them are declared in
include/lz4m.h, exported by the library and bound in lz4/_native.py."""
import os
import re

import pytest

from conftest import ROOT

import lz4.frame

HEADER = os.path.join(ROOT, "include", "lz4m.h")
NEW_CALLS = ["lz4m_frames_scan", "lz4m_frames_records", "lz4m_decompress_chains", "lz4m_frames_plan",
             "lz4m_frames_plan_blocks", "lz4m_frames_sizes", "lz4m_frames_emit"]


def test_names_are_exported():
    for name in ("compress_batch", "decompress_batch", "compress_many", "decompress_many"):
        assert callable(getattr(lz4.frame, name)), name


def test_empty_lists_touch_no_device():
    assert lz4.frame.compress_many([]) == []
    assert lz4.frame.decompress_many([]) == []
    assert lz4.frame.compress_many((), content_checksum=True, block_linked=False) == []
    assert lz4.frame.decompress_many((), return_bytes_read=True) == []


def _raised(fn, *a, **k):
    with pytest.raises(Exception) as e:
        fn(*a, **k)
    return type(e.value), str(e.value)


@pytest.mark.parametrize("bad", ["text", 1.5, None, 7], ids=["str", "float", "none", "int"])
def test_wrong_data_type_raises_what_the_single_call_raises(bad):
    assert _raised(lz4.frame.compress_many, [bad]) == _raised(lz4.frame.compress, bad)
    assert _raised(lz4.frame.compress_many, [b"fine", bad]) == _raised(lz4.frame.compress, bad)
    assert _raised(lz4.frame.decompress_many, [bad]) == _raised(lz4.frame.decompress, bad)


def test_not_a_list_raises():
    with pytest.raises(TypeError):
        lz4.frame.compress_many(5)
    with pytest.raises(TypeError):
        lz4.frame.decompress_many(None)


@pytest.mark.parametrize("kw", [{"compression_level": "3"}, {"compression_level": 1.0}, {"block_size": "4"},
                                {"block_size": None}, {"compression_level": 1 << 31}, {"block_size": -(1 << 31) - 1},
                                {"compression_level": 1 << 40}])
def test_wrong_or_out_of_range_options_raise_what_the_single_call_raises(kw):
    """The integer options are converted before any device work, as in
    compress: the wrong type and a value outside the C int range."""
    single = _raised(lz4.frame.compress, b"abc", **kw)
    assert single[0] in (TypeError, OverflowError)
    assert _raised(lz4.frame.compress_many, [b"abc"], **kw) == single
    assert _raised(lz4.frame.compress_many, [], **kw) == single


def test_device_calls_check_their_arguments_first():
    """compress_batch's parse / level errors are compress_device's, raised before the tensors are looked at."""
    for kw in ({"parse": "fast"}, {"parse": "hc", "compression_level": 2}, {"compression_level": 3},
               {"parse": "parallel", "compression_level": 9}):
        assert (_raised(lz4.frame.compress_batch, None, None, None, **kw)
                == _raised(lz4.frame.compress_device, None, 0, **kw))


def _declared():
    txt = open(HEADER).read()
    return set(re.findall(r"^\s*(?:[\w\s\*]+?)\b(lz4m_\w+)\s*\(", txt, re.M))


def test_new_calls_are_declared_exported_and_bound():
    from lz4 import _native as N
    declared = _declared()
    lib = N.lib()
    for name in NEW_CALLS:
        assert name in declared, f"{name} missing from include/lz4m.h"
        assert hasattr(lib, name), f"{name} not exported by the library"
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is not None, f"{name} not declared in lz4/_native.py"


def test_every_frames_call_in_the_header_is_bound():
    """Whatever include/lz4m.h declares for batched frames is in the list above (nothing unbound slips in)."""
    from lz4 import _native as N
    lib = N.lib()
    for name in sorted(_declared()):
        if name.startswith("lz4m_frames_") or name == "lz4m_decompress_chains":
            assert name in NEW_CALLS, name
            assert getattr(lib, name).argtypes is not None, name


def test_empty_and_negative_batches_need_no_device():
    from lz4 import _native as N
    lib = N.lib()
    z = [None] * 20
    assert lib.lz4m_frames_scan(*z[:3], 0, *z[:8], None) == 0
    assert lib.lz4m_frames_scan(*z[:3], -1, *z[:8], None) == N.EINVAL
    assert lib.lz4m_frames_scan(*z[:3], 4, *z[:8], None) == N.EINVAL          # null arrays
    assert lib.lz4m_frames_records(*z[:9], 0, *z[:7], None) == 0
    assert lib.lz4m_frames_records(*z[:9], -1, *z[:7], None) == N.EINVAL
    assert lib.lz4m_decompress_chains(*z[:10], 0, None) == 0
    assert lib.lz4m_decompress_chains(*z[:10], -1, None) == N.EINVAL
    assert lib.lz4m_decompress_chains(*z[:10], 3, None) == N.EINVAL
    assert lib.lz4m_frames_plan(None, 0, 4, 1, None, None, None, None) == 0
    assert lib.lz4m_frames_plan(None, -1, 4, 1, None, None, None, None) == N.EINVAL
    assert lib.lz4m_frames_plan_blocks(*z[:5], 1, 0, *z[:7], None) == 0
    assert lib.lz4m_frames_plan_blocks(*z[:5], 1, -1, *z[:7], None) == N.EINVAL
    assert lib.lz4m_frames_sizes(None, None, None, 1, 1, 0, None, None, None) == 0
    assert lib.lz4m_frames_sizes(None, None, None, 1, 1, -1, None, None, None) == N.EINVAL
    assert lib.lz4m_frames_emit(*z[:6], 1, 0, 0, None, 0, None) == 0
    assert lib.lz4m_frames_emit(*z[:6], 1, 0, 0, None, -1, None) == N.EINVAL

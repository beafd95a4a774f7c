"""Shared pieces of tests/test_opt_model.py and tests/test_gpu_opt.py: the CPU
model of the optimal parse (tests/hc_model/opt_model.c, built with gcc into
hc_support's temporary directory on first use).  The inputs are hc_support's."""
import ctypes as C
import functools

import numpy as np

import hc_support as H

ALL_KINDS = H.KINDS + ("runs", "random")


@functools.lru_cache(maxsize=None)
def model_lib():
    lib = H._build(H.OPT_MODEL_C, "libopt_model.so")
    lib.opt_model_compress.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
    lib.opt_model_compress.restype = C.c_int
    lib.opt_model_cost.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.opt_model_cost.restype = C.c_int
    return lib


@functools.lru_cache(maxsize=None)
def _compress_full(data: bytes, level: int) -> bytes:
    src = H._array(data)
    cap = H.compress_bound(src.size)
    dst = np.zeros(cap, dtype=np.uint8)
    r = model_lib().opt_model_compress(src.ctypes.data if src.size else None, src.size, dst.ctypes.data, cap, level)
    assert r > 0
    return dst[:r].tobytes()


def model_compress(data, level: int, cap: int | None = None) -> bytes | None:
    """The model's block for ``data`` (None when it does not fit ``cap``).
    Blocks at the full bound are computed once per (data, level) and shared."""
    if cap is None:
        return _compress_full(bytes(data), level)
    src = H._array(data)
    dst = np.full(cap + 1, 0xA5, dtype=np.uint8)
    r = model_lib().opt_model_compress(src.ctypes.data if src.size else None, src.size, dst.ctypes.data, cap, level)
    assert dst[cap] == 0xA5   # nothing past the capacity
    return None if r <= 0 else dst[:r].tobytes()


def model_cost(data, level: int) -> int:
    """cost[0] of the model's price pass."""
    src = H._array(data)
    return model_lib().opt_model_cost(src.ctypes.data if src.size else None, src.size, level)

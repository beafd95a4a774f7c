"""Shared pieces of tests/test_hc_model.py and tests/test_gpu_hc.py: the CPU
model of the HC parse (tests/hc_model/hc_model.c, built with gcc into a
temporary directory on first use) and the edge-case inputs both files use."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

MODEL_DIR = os.path.join(ROOT, "tests", "hc_model")
MODEL_C = os.path.join(MODEL_DIR, "hc_model.c")
CHECK_C = os.path.join(MODEL_DIR, "hc_model_check.c")

LENGTHS = (0, 1, 4, 5, 11, 12, 13, 14, 16, 17, 64, 65535, 65536, 65537, 200003)
KINDS = ("text", "source", "markup", "records", "silesia")


@functools.lru_cache(maxsize=None)
def build_dir() -> str:
    d = tempfile.mkdtemp(prefix="hc_model_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


@functools.lru_cache(maxsize=None)
def model_lib():
    so = os.path.join(build_dir(), "libhc_model.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-fPIC", "-shared", MODEL_C, "-o", so],
                   check=True, capture_output=True, text=True)
    lib = C.CDLL(so)
    lib.hc_model_compress.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
    lib.hc_model_compress.restype = C.c_int
    return lib


def compress_bound(n: int) -> int:
    return n + n // 255 + 16


def model_compress(data, level: int, cap: int | None = None) -> bytes | None:
    """The model's block for ``data`` (None when it does not fit ``cap``)."""
    src = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data)
    cap = compress_bound(src.size) if cap is None else cap
    dst = np.zeros(max(cap, 1), dtype=np.uint8)
    r = model_lib().hc_model_compress(src.ctypes.data if src.size else None, src.size, dst.ctypes.data, cap, level)
    return None if r <= 0 else dst[:r].tobytes()


@functools.lru_cache(maxsize=None)
def validity_inputs() -> tuple:
    """(name, bytes) for every length of LENGTHS x {zeros, a repeated pattern
    of period 1/2/3/4/7, random bytes, synthetic text}, plus 70000 zeros (long
    runs of 255 in the match length)."""
    from lz4 import _synth
    rng = np.random.default_rng(20261019)
    top = max(LENGTHS)
    rnd = rng.integers(0, 256, size=top, dtype=np.uint8).tobytes()
    text = _synth.word_text(np.random.default_rng(5), top).tobytes()
    out = []
    for n in LENGTHS:
        out.append((f"zeros-{n}", bytes(n)))
        for period in (1, 2, 3, 4, 7):
            unit = bytes(range(0x41, 0x41 + period))
            out.append((f"period{period}-{n}", (unit * (n // period + 1))[:n]))
        out.append((f"random-{n}", rnd[:n]))
        out.append((f"text-{n}", text[:n]))
    out.append(("zeros-70000", bytes(70000)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def window_inputs() -> tuple:
    """A random unit of 65535 / 65536 / 65537 bytes repeated to 3 * period +
    1000 bytes: only the first is within LZ4_DISTANCE_MAX."""
    out = []
    for period in (65535, 65536, 65537):
        unit = np.random.default_rng(period).integers(0, 256, size=period, dtype=np.uint8).tobytes()
        n = 3 * period + 1000
        out.append((period, (unit * 4)[:n]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def kind_blocks(kind: str) -> tuple:
    from lz4 import _synth
    return tuple(b.tobytes() for b in _synth.blocks(24, kind, seed=31))

"""Shared pieces of the tests of the hash-chain parses (HC, HC with a prefix,
optimal; hc_prefix_support and opt_support build on this module): the CPU
models of tests/hc_model/, built with gcc into a temporary directory on first
use, their stand-alone check program, the edge-case inputs, and the helpers of
the GPU test files (torch and the package are imported where they are used, so
the CPU tests need neither a GPU nor the native library)."""
import atexit
import ctypes as C
import functools
import os
import shutil
import re
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

MODEL_DIR = os.path.join(ROOT, "tests", "hc_model")
MODEL_C = os.path.join(MODEL_DIR, "hc_model.c")
OPT_MODEL_C = os.path.join(MODEL_DIR, "opt_model.c")   # includes hc_model.c
CHECK_C = os.path.join(MODEL_DIR, "model_check.c")

LENGTHS = (0, 1, 4, 5, 11, 12, 13, 14, 16, 17, 64, 65535, 65536, 65537, 200003)
KINDS = ("text", "source", "markup", "records", "silesia")


@functools.lru_cache(maxsize=None)
def build_dir() -> str:
    d = tempfile.mkdtemp(prefix="hc_model_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def _build(source: str, name: str):
    """``source`` as the shared object ``name`` in build_dir(), loaded."""
    so = os.path.join(build_dir(), name)
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-fPIC", "-shared", source, "-o", so],
                   check=True, capture_output=True, text=True)
    return C.CDLL(so)


def _array(data) -> np.ndarray:
    return np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data)


@functools.lru_cache(maxsize=None)
def model_lib():
    """hc_model.c: the HC parse, without and with a prefix."""
    lib = _build(MODEL_C, "libhc_model.so")
    lib.hc_model_compress.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int]
    lib.hc_model_compress.restype = C.c_int
    lib.hc_model_compress_prefix.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    lib.hc_model_compress_prefix.restype = C.c_int
    return lib


@functools.lru_cache(maxsize=None)
def check_program():
    """model_check (its own main, ASan + UBSan) built and run once: it runs the
    three models over their edge cases with exactly sized buffers, prints one
    "<model>_check: ok" line per model and exits 0.  Returns the finished run."""
    exe = os.path.join(build_dir(), "model_check")
    r = subprocess.run(["gcc", "-O2", "-g", "-std=c99", "-Wall", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", CHECK_C, OPT_MODEL_C,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))


def compress_bound(n: int) -> int:
    return n + n // 255 + 16


def model_compress(data, level: int, cap: int | None = None) -> bytes | None:
    """The model's block for ``data`` (None when it does not fit ``cap``)."""
    src = _array(data)
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


# ------------------------------------------------- helpers of the GPU tests
def pack(blocks, dev, first: int = 0, gap: int = 0):
    """Blocks back to back (``gap`` bytes between them, the first at offset ``first``)."""
    import torch
    lens = np.array([len(b) for b in blocks], dtype=np.int32)
    offs = np.full(len(blocks), first, dtype=np.int64)
    offs[1:] += np.cumsum(lens[:-1].astype(np.int64) + gap)
    buf = np.zeros(int(offs[-1] + lens[-1]) + 16, dtype=np.uint8)
    for b, o in zip(blocks, offs):
        buf[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return torch.from_numpy(buf).to(dev), torch.from_numpy(offs).to(dev), torch.from_numpy(lens).to(dev)


def outputs(dst, dst_off, out_len):
    d, o, n = dst.cpu().numpy(), dst_off.cpu().numpy(), out_len.cpu().numpy()
    return [d[int(a):int(a) + int(k)].tobytes() for a, k in zip(o, n)]


def assert_decodes(src, ln, dst, dst_off, out_len):
    """Every block decodes on the device to its input (blocks packed back to back in src)."""
    import torch

    import lz4.block
    assert bool((out_len > 0).all())
    back, _, status = lz4.block.decompress_batch(dst, dst_off, out_len, ln)
    assert torch.equal(status, ln)
    total = int(ln.sum().item())
    assert torch.equal(back[:total], src[:total])


def mixed_batch() -> list:
    """4096 blocks of 0..70000 bytes cut from the silesia mix (seeded)."""
    from lz4 import _synth
    pool = _synth.blocks(256, "silesia", seed=77, block=70000)
    rng = np.random.default_rng(4096)
    lens = rng.integers(0, 70001, size=4096)
    lens[:4] = (0, 70000, 13, 12)
    return [pool[i % 256, :int(n)].tobytes() for i, n in enumerate(lens)]


def scratch_report(name: str) -> list:
    """[(kernel, scratch bytes per lane)] of the compiler's resource report
    build/``name`` that the csrc Makefile keeps next to each object."""
    csrc = os.path.join(ROOT, "python-lz4_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc], check=True, capture_output=True)
    rep = os.path.join(csrc, "build", name)
    assert os.path.exists(rep), os.listdir(os.path.join(csrc, "build"))
    out, kernel = [], None
    for line in open(rep):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            kernel = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and kernel:
            out.append((kernel, int(m.group(1))))
    return out

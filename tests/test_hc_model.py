"""CPU tests of the HC parse's model (tests/hc_model/hc_model.c): the serial
definition of DESIGN.md section 9 that lz4m_compress_hc_batch reproduces byte
for byte (tests/test_gpu_hc.py).  Validity against the oracle's decoder, the
window's edge, sizes against the reference's LZ4_compress_HC, and a
sanitizer run of the stand-alone check program."""
import ctypes as C
import json
import os

import pytest

import hc_support as H
from conftest import GOLDEN

SIZES = json.load(open(os.path.join(GOLDEN, "hc_sizes.json")))["reference"]

# The model's measured total / the reference's LZ4_compress_HC total at the
# same level over _synth.blocks(24, kind, seed=31), rounded up to the next
# 0.5 % (DESIGN.md section 9 lists both):
#   level 4: text 1.02157, source 1.02826, markup 1.00503, records 1.00047, silesia 1.01375
#   level 9: text 1.01724, source 1.02318, markup 1.00516, records 1.00008, silesia 1.01110
BARS = {
    4: {"text": 1.025, "source": 1.030, "markup": 1.010, "records": 1.005, "silesia": 1.015},
    9: {"text": 1.020, "source": 1.025, "markup": 1.010, "records": 1.005, "silesia": 1.015},
}
COMPRESSIBLE = ("text", "source", "markup", "records")


def _roundtrip(oracle, data: bytes, level: int) -> bytes:
    comp = H.model_compress(data, level)
    assert comp is not None and len(comp) <= H.compress_bound(len(data))
    r, back = oracle.decompress(comp, len(data))
    assert r == len(data) and back == data
    return comp


@pytest.mark.parametrize("level", [3, 9])
def test_model_output_is_valid(oracle, level):
    for name, data in H.validity_inputs():
        try:
            _roundtrip(oracle, data, level)
        except AssertionError:
            raise AssertionError(f"{name} at level {level}")
    assert H.model_compress(b"", level) == b"\x00"
    for n in (1, 4, 5, 11, 12):   # below 13 bytes: one literal run
        data = bytes(range(n))
        assert H.model_compress(data, level) == bytes([n << 4]) + data


def test_model_long_match_length_bytes(oracle):
    comp = _roundtrip(oracle, bytes(70000), 9)
    assert comp.count(b"\xff" * 200) >= 1 and len(comp) < 300


def test_model_limited_output():
    for name, data in H.validity_inputs():
        if len(data) > 70000:
            continue
        full = H.model_compress(data, 4)
        assert H.model_compress(data, 4, cap=len(full)) == full, name
        assert H.model_compress(data, 4, cap=len(full) - 1) is None, name
        assert H.model_compress(data, 4, cap=0) is None, name


def test_model_window_edge(oracle):
    """Offsets stop at 65535 (LZ4_DISTANCE_MAX): only the 65535-byte period is found."""
    for period, data in H.window_inputs():
        comp = _roundtrip(oracle, data, 4)
        if period == 65535:
            assert len(comp) < period + 4096
        else:
            assert len(comp) > len(data)   # nothing within reach: stored as literals


@pytest.fixture(scope="module")
def model_totals():
    kinds = H.KINDS + ("runs", "random")
    return {lvl: {k: sum(len(H.model_compress(b, lvl)) for b in H.kind_blocks(k)) for k in kinds} for lvl in (4, 9)}


def test_bars_respect_the_caps():
    for lvl in (4, 9):
        for kind, bar in BARS[lvl].items():
            assert bar <= (1.03 if kind == "silesia" else 1.05), (lvl, kind)


@pytest.mark.parametrize("level", [4, 9])
def test_model_sizes_against_reference_hc(model_totals, level):
    for kind in H.KINDS:
        got, ref = model_totals[level][kind], SIZES[kind][f"hc{level}"]
        print(f"level {level} {kind}: model {got} reference {ref} ratio {got / ref:.5f} bar {BARS[level][kind]}")
        assert got <= BARS[level][kind] * ref, (kind, got, ref)


def test_model_sizes_order(model_totals, oracle):
    for kind in COMPRESSIBLE:
        assert model_totals[9][kind] <= model_totals[4][kind], kind
        default = sum(len(oracle.compress(b)) for b in H.kind_blocks(kind))
        assert model_totals[4][kind] < default, kind
    for kind in ("runs", "random"):
        for lvl in (4, 9):
            assert model_totals[lvl][kind] <= 1.005 * SIZES[kind]["default"], (kind, lvl)


def test_golden_sizes_match_reference_build():
    """tests/golden/hc_sizes.json holds what the reference build computes
    (compared where that build is present; the JSON stands in where it is not)."""
    import oracle as O
    if not os.path.exists(O.REF_SO):
        return
    ref = C.CDLL(O.REF_SO)
    ref.LZ4_compress_HC.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    ref.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    for kind, row in SIZES.items():
        tot = {"hc4": 0, "hc9": 0, "default": 0}
        for b in H.kind_blocks(kind):
            dst = C.create_string_buffer(H.compress_bound(len(b)))
            tot["hc4"] += ref.LZ4_compress_HC(b, dst, len(b), len(dst), 4)
            tot["hc9"] += ref.LZ4_compress_HC(b, dst, len(b), len(dst), 9)
            tot["default"] += ref.LZ4_compress_default(b, dst, len(b), len(dst))
        assert tot == row, kind


def test_model_check_program_under_sanitizers():
    """model_check (its own main, ASan + UBSan; one run shared by the three
    model test files) runs the HC model over the
    edge cases with exactly sized buffers and exits 0."""
    r = H.check_program()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hc_model_check: ok" in r.stdout

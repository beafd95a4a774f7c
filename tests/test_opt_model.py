"""CPU tests of the optimal parse's model (tests/hc_model/opt_model.c): the
serial definition of DESIGN.md section 9.7 that lz4m_compress_opt_batch
reproduces byte for byte (tests/test_gpu_opt.py).  Validity against the
oracle's decoder, the size against the price pass, the window's edge, sizes
against the reference's LZ4_compress_HC(12) and against the HC model, and a
sanitizer run of the stand-alone check program."""
import ctypes as C
import json
import os

import pytest

import hc_support as H
import opt_support as P
from conftest import GOLDEN

SIZES = json.load(open(os.path.join(GOLDEN, "opt_sizes.json")))["reference"]

# The model's measured level-9 total / the reference's LZ4_compress_HC(12)
# total over _synth.blocks(24, kind, seed=31), rounded up to the next 0.5 %
# (DESIGN.md section 9.7 lists both):
#   text 1.00081, source 1.00389, markup 1.00650, records 1.00207,
#   silesia 1.00176, runs 1.02313
BARS = {"text": 1.005, "source": 1.005, "markup": 1.010, "records": 1.005, "silesia": 1.005, "runs": 1.025}
CAPS = {"text": 1.01, "source": 1.01, "markup": 1.01, "records": 1.01, "silesia": 1.01, "runs": 1.03}
SMALLER_THAN_HC = ("text", "source", "markup", "silesia")
COMPRESSIBLE = ("text", "source", "markup", "records")


def _roundtrip(oracle, data: bytes, level: int) -> bytes:
    comp = P.model_compress(data, level)
    assert comp is not None and len(comp) <= H.compress_bound(len(data))
    r, back = oracle.decompress(comp, len(data))
    assert r == len(data) and back == data
    assert len(comp) == P.model_cost(data, level)   # the emitted size is cost[0]
    return comp


@pytest.mark.parametrize("level", [3, 9])
def test_model_output_is_valid(oracle, level):
    for name, data in H.validity_inputs():
        try:
            _roundtrip(oracle, data, level)
        except AssertionError:
            raise AssertionError(f"{name} at level {level}")
    assert P.model_compress(b"", level) == b"\x00"
    for n in (1, 4, 5, 11, 12):   # below 13 bytes: one literal run
        data = bytes(range(n))
        assert P.model_compress(data, level) == bytes([n << 4]) + data


def test_model_long_match_length_bytes(oracle):
    comp = _roundtrip(oracle, bytes(70000), 9)
    assert comp.count(b"\xff" * 200) >= 1 and len(comp) < 300


def test_model_limited_output():
    for name, data in H.validity_inputs():
        if len(data) > 70000:
            continue
        full = P.model_compress(data, 3)
        assert P.model_compress(data, 3, cap=len(full)) == full, name
        assert P.model_compress(data, 3, cap=len(full) - 1) is None, name
        assert P.model_compress(data, 3, cap=0) is None, name


@pytest.mark.parametrize("level", [3, 9])
def test_model_window_edge(oracle, level):
    """Offsets stop at 65535 (LZ4_DISTANCE_MAX): only the 65535-byte period is found."""
    for period, data in H.window_inputs():
        comp = _roundtrip(oracle, data, level)
        if period == 65535:
            assert len(comp) < period + 4096
        else:
            assert len(comp) > len(data)   # nothing within reach: stored as literals


@pytest.fixture(scope="module")
def totals():
    opt = {lvl: {k: sum(len(P.model_compress(b, lvl)) for b in H.kind_blocks(k)) for k in P.ALL_KINDS}
           for lvl in (4, 9)}
    hc9 = {k: sum(len(H.model_compress(b, 9)) for b in H.kind_blocks(k)) for k in P.ALL_KINDS}
    return opt, hc9


def test_bars_respect_the_caps():
    assert set(BARS) == set(CAPS)
    for kind, bar in BARS.items():
        assert bar <= CAPS[kind], kind


def test_model_sizes_against_reference_level_12(totals):
    opt, _ = totals
    for kind, bar in BARS.items():
        got, ref = opt[9][kind], SIZES[kind]["hc12"]
        print(f"{kind}: model {got} reference level 12 {ref} ratio {got / ref:.5f} bar {bar}")
        assert got <= bar * ref, (kind, got, ref)
    assert opt[9]["random"] <= SIZES["random"]["hc12"]


def test_model_sizes_against_the_hc_model(totals):
    opt, hc9 = totals
    for kind in P.ALL_KINDS:
        print(f"{kind}: optimal {opt[9][kind]} hc model {hc9[kind]} ratio {opt[9][kind] / hc9[kind]:.5f}")
    for kind in SMALLER_THAN_HC:
        assert opt[9][kind] < hc9[kind], kind
    for kind in ("records", "runs", "random"):
        assert opt[9][kind] <= 1.005 * hc9[kind], kind
    for kind in COMPRESSIBLE:
        assert opt[9][kind] <= opt[4][kind], kind


def test_golden_sizes_match_reference_build():
    """tests/golden/opt_sizes.json holds what the reference build computes
    (compared where that build is present; the JSON stands in where it is not)."""
    import oracle as O
    if not os.path.exists(O.REF_SO):
        return
    ref = C.CDLL(O.REF_SO)
    ref.LZ4_compress_HC.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    assert set(SIZES) == set(P.ALL_KINDS)
    for kind, row in SIZES.items():
        tot = {f"hc{lvl}": 0 for lvl in (9, 10, 11, 12)}
        for b in H.kind_blocks(kind):
            dst = C.create_string_buffer(H.compress_bound(len(b)))
            for lvl in (9, 10, 11, 12):
                tot[f"hc{lvl}"] += ref.LZ4_compress_HC(b, dst, len(b), len(dst), lvl)
        assert tot == row, kind


def test_model_check_program_under_sanitizers():
    """model_check (its own main, ASan + UBSan; one run shared by the three
    model test files) runs the optimal model over
    the edge cases with exactly sized buffers and exits 0."""
    r = H.check_program()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "opt_model_check: ok" in r.stdout

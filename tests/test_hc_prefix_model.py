"""CPU tests of the model of the HC parse with a prefix
(hc_model_compress_prefix of tests/hc_model/hc_model.c): the serial definition of DESIGN.md section
9.5 that lz4m_compress_hc_dict_batch reproduces byte for byte
(tests/test_gpu_hc_prefix.py).  An empty prefix gives the old model's bytes;
validity against the oracle's decoder with the prefix as dictionary; the edge
cases of the prefix; limited output; a sanitizer run of the stand-alone check
program; sizes of linked frames against the reference's LZ4F_compressFrame."""
import json
import os

import pytest

import hc_prefix_support as HP
import hc_support as H
from conftest import GOLDEN

SIZES = json.load(open(os.path.join(GOLDEN, "hc_prefix_sizes.json")))["reference"]

# The model's measured payload / the reference's LZ4F_compressFrame payload at
# the same level, over b"".join(_synth.blocks(24, kind, seed=31)) as one frame
# of linked 64 KiB blocks, rounded up to the next 0.5 % (DESIGN.md section 9.5
# lists both):
#   level 4: text 1.03620, source 1.04892, markup 1.00995, records 1.00078, silesia 1.01695
#   level 9: text 1.02848, source 1.03825, markup 1.01109, records 1.00009, silesia 1.01363
BARS = {
    4: {"text": 1.040, "source": 1.050, "markup": 1.010, "records": 1.005, "silesia": 1.020},
    9: {"text": 1.030, "source": 1.040, "markup": 1.015, "records": 1.005, "silesia": 1.015},
}
# The model's linked payload / its payload for independent blocks:
#   level 4: text 0.90186, source 0.89392, markup 0.93674, records 0.99141, silesia 0.97537
#   level 9: text 0.88266, source 0.87379, markup 0.93220, records 0.99066, silesia 0.97087
# The prefix pays (>= 2.4 %) on these kinds; on `records` it gains under 1 %, which is not asserted.
LINKED_GAINS = ("text", "source", "markup", "silesia")


def _roundtrip(oracle, prefix: bytes, block: bytes, level: int) -> bytes:
    comp = HP.model_compress_prefix(prefix, block, level)
    assert comp is not None and len(comp) <= H.compress_bound(len(block))
    r, back = oracle.decompress(comp, len(block), dict_=prefix)
    assert r == len(block) and back == block
    return comp


@pytest.mark.parametrize("level", [3, 9])
def test_empty_prefix_equals_the_old_model(level):
    inputs = list(H.validity_inputs()) + [(f"window-{p}", d) for p, d in H.window_inputs()]
    for kind in H.KINDS:
        inputs += [(f"{kind}-{i}", b) for i, b in enumerate(H.kind_blocks(kind))]
    for name, data in inputs:
        assert HP.model_compress_prefix(b"", data, level) == H.model_compress(data, level), name


@pytest.mark.parametrize("level", [3, 9])
def test_model_output_is_valid(oracle, level):
    for name, prefix, block in HP.grid_cases():
        try:
            comp = _roundtrip(oracle, prefix, block, level)
        except AssertionError:
            raise AssertionError(f"{name} at level {level}")
        if len(block) == 0:
            assert comp == b"\x00", name
        elif len(block) < 13:   # one literal run
            assert comp == bytes([len(block) << 4]) + block, name


def test_window_edge(oracle):
    """Distance 65535 (LZ4_DISTANCE_MAX) reaches into the prefix, 65536 does not."""
    prefix, block = HP.edge_cases()["dist65535"]
    comp = _roundtrip(oracle, prefix, block, 4)
    assert len(comp) < len(block) - 900
    assert comp[:4] == b"\x0f\xff\xff\xff"   # no literal, a long match at offset 65535
    prefix, block = HP.edge_cases()["dist65536"]
    comp = _roundtrip(oracle, prefix, block, 4)
    assert len(comp) > len(block)


def test_backward_extension_stops_at_the_block_start(oracle):
    """Prefix P Q filler P, block Q random: the bytes before the match and
    before its source are equal, but the match may not start in the prefix."""
    prefix, block = HP.edge_cases()["back_stop"]
    for level in (3, 9):
        comp = _roundtrip(oracle, prefix, block, level)
        assert comp[0] >> 4 == 0                                   # no literals: the match starts the block
        assert int.from_bytes(comp[1:3], "little") == 100 + 500 + 100   # from Q in the prefix
        assert (comp[0] & 15) == 15 and 4 + 15 + comp[3] == 100    # all of Q, nothing more


def test_run_across_the_boundary(oracle):
    prefix, block = HP.edge_cases()["run"]
    comp = _roundtrip(oracle, prefix, block, 9)
    assert len(comp) < 16 and comp[0] >> 4 == 0 and comp[1:3] == b"\x01\x00"   # offset 1, overlapping the boundary


def test_short_block_is_literals(oracle):
    prefix, _ = HP.edge_cases()["short"]
    for n in (1, 4, 11, 12):
        block = prefix[:n]   # a perfect match in the prefix
        assert _roundtrip(oracle, prefix, block, 9) == bytes([n << 4]) + block
    assert _roundtrip(oracle, prefix, b"", 9) == b"\x00"
    assert len(_roundtrip(oracle, prefix, prefix[:13], 9)) == 9   # 13 bytes: a match of 8 (to n - 5), 5 literals


def test_model_limited_output():
    cases = [(n, p, b) for n, p, b in HP.grid_cases() if len(p) in (7, 4096, 65536) and len(b) <= 65536]
    cases += [(name, p, b) for name, (p, b) in HP.edge_cases().items()]
    for name, prefix, block in cases:
        full = HP.model_compress_prefix(prefix, block, 4)
        assert HP.model_compress_prefix(prefix, block, 4, cap=len(full)) == full, name
        assert HP.model_compress_prefix(prefix, block, 4, cap=len(full) - 1) is None, name
        assert HP.model_compress_prefix(prefix, block, 4, cap=0) is None, name


def test_model_check_program_under_sanitizers():
    """model_check (its own main, ASan + UBSan; one run shared by the three
    model test files) runs the prefix model over
    prefixes and blocks in exactly sized buffers and exits 0."""
    r = H.check_program()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hc_model_prefix_check: ok" in r.stdout



@pytest.fixture(scope="module")
def frame_totals():
    """level -> kind -> (linked payload, independent payload) of the model."""
    out = {}
    for lvl in (4, 9):
        out[lvl] = {}
        for kind in H.KINDS:
            data = b"".join(H.kind_blocks(kind))
            out[lvl][kind] = tuple(sum(len(p) for p in HP.linked_frame_parts(data, lvl, linked))
                                   for linked in (True, False))
    return out


def test_bars_respect_the_caps():
    for lvl in (4, 9):
        for kind, bar in BARS[lvl].items():
            assert bar <= (1.03 if kind == "silesia" else 1.05), (lvl, kind)


@pytest.mark.parametrize("level", [4, 9])
def test_linked_frame_sizes_against_reference(frame_totals, level):
    for kind in H.KINDS:
        got, ref = frame_totals[level][kind][0], SIZES[kind][f"payload{level}"]
        print(f"level {level} {kind}: model {got} reference {ref} ratio {got / ref:.5f} bar {BARS[level][kind]}")
        assert got <= BARS[level][kind] * ref, (kind, got, ref)


@pytest.mark.parametrize("level", [4, 9])
def test_linked_is_smaller_than_independent(frame_totals, level):
    for kind in H.KINDS:
        linked, indep = frame_totals[level][kind]
        print(f"level {level} {kind}: linked {linked} independent {indep} ratio {linked / indep:.5f}")
    for kind in LINKED_GAINS:
        linked, indep = frame_totals[level][kind]
        assert linked <= indep, kind


def test_golden_sizes_match_reference_build():
    """tests/golden/hc_prefix_sizes.json holds what the reference build computes
    (compared where that build is present; the JSON stands in where it is not)."""
    import oracle as O
    if not os.path.exists(O.REF_SO):
        return
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_hc_prefix_sizes",
                                                  os.path.join(GOLDEN, "make_hc_prefix_sizes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.reference_sizes(O.Reference()) == SIZES

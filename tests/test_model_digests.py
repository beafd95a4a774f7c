"""The output bytes of the CPU models of tests/hc_model/ (HC, HC with a
prefix, optimal) against tests/golden/model_digests.json, which
tests/golden/make_model_digests.py wrote: sizes and one SHA-256 per (model,
input family, level), and the limited-output behaviour per model.  The models
define the kernels' bytes (test_kernel_bytes_equal_the_model), so this is what
"the models' behaviour is unchanged" means."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

MODELS = ("hc", "prefix", "opt")


@pytest.fixture(scope="module")
def computed():
    spec = importlib.util.spec_from_file_location("make_model_digests", os.path.join(GOLDEN, "make_model_digests.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen.compute()


@pytest.fixture(scope="module")
def pinned():
    return json.load(open(os.path.join(GOLDEN, "model_digests.json")))


def _compare(where: str, got: dict, want: dict):
    names = got["cases"]
    assert len(got["sizes"]) == len(want["sizes"]), f"{where}: {len(got['sizes'])} cases, not {len(want['sizes'])}"
    for name, g, w in zip(names, got["sizes"], want["sizes"]):
        assert g == w, f"{where}: {name} gives {g} bytes, not {w}"
    assert got["sha256"] == want["sha256"], f"{where}: the sizes agree, the bytes differ"


@pytest.mark.parametrize("model", MODELS)
def test_model_bytes_are_the_pinned_ones(computed, pinned, model):
    assert set(computed[model]) == set(pinned[model])
    for family, levels in computed[model].items():
        assert set(levels) == set(pinned[model][family]), family
        for level, got in levels.items():
            _compare(f"{model} model, family {family}, level {level}", got, pinned[model][family][level])


@pytest.mark.parametrize("model", MODELS)
def test_model_limited_output_is_the_pinned_one(computed, pinned, model):
    got, want = computed["capacity"][model], pinned["capacity"][model]
    assert got["level"] == want["level"]
    _compare(f"{model} model, capacity cases, level {got['level']}", got, want)
    for name, same, short, zero in zip(got["cases"], got["same_at_size"], got["at_size_minus_1"], got["at_zero"]):
        assert same, f"{model} model: {name} at cap = size gives other bytes"
        assert short == 0 and zero == 0, f"{model} model: {name} is not refused at cap = size - 1 or cap = 0"
    for key in ("same_at_size", "at_size_minus_1", "at_zero"):
        assert got[key] == want[key], (model, key)

"""The bytes of the frame and block compression calls against
tests/golden/frame_digests.json, which tests/golden/make_frame_digests.py
wrote on the commit before the frame calls came to share one block stage, one
parse resolver and one launch function: sizes and one SHA-256 per case.  The
batched calls promise the single calls' bytes; this pins both to what they
were, not to each other."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# the cases in groups of a few seconds each: by the word that follows the call's name
GROUPS = {"frame": ["exact", "parallel bs0", "parallel bs5", "parallel bs7", "hc4", "hc9", "optimal9", "default"],
          "block": [""]}


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_frame_digests", os.path.join(GOLDEN, "make_frame_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "frame_digests.json")) as f:
        return json.load(f)


def _in_group(name: str, key: str) -> bool:
    return name.split(" ", 1)[1].startswith(key)


def test_groups_cover_every_pinned_case(pinned):
    for group, keys in GROUPS.items():
        for name in pinned[group]:
            assert sum(_in_group(name, k) for k in keys) == 1, name


@pytest.mark.parametrize("group,key", [(g, k) for g, keys in GROUPS.items() for k in keys])
def test_bytes_are_the_pinned_ones(gpu, gen, pinned, group, key):
    want = {n: e for n, e in pinned[group].items() if _in_group(n, key)}
    got = gen.compute(lambda g, n: g == group and _in_group(n, key))[group]
    assert set(got) == set(want) and want
    for name, w in want.items():
        g = got[name]
        if "decodes" in w:
            assert g["decodes"], f"{name}: the output does not decode to the input"
        if "sizes" in w:
            assert g["sizes"] == w["sizes"], f"{name}: sizes {g['sizes']}, not {w['sizes']}"
        if "sha256" in w:
            assert g["sha256"] == w["sha256"], f"{name}: the sizes agree, the bytes differ"

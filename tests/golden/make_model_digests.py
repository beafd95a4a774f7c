"""Writes tests/golden/model_digests.json: the output bytes of the three CPU
models of tests/hc_model/ (HC, HC with a prefix, optimal), pinned as sizes and
digests.  Per (model, input family, level): the output sizes, one per case in
the family's order, and one SHA-256 over the outputs concatenated in that
order, each preceded by its LE32 length.  Per model, the limited-output
behaviour on hc_support.validity_inputs() of at most 70000 bytes: the same
bytes at cap = size, a result of 0 at cap = size - 1 and at cap = 0.  Needs
only gcc; run from the repository root:
    python tests/golden/make_model_digests.py
tests/test_model_digests.py recomputes all of it and compares: a change to a
model that moves one output byte shows there."""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (conftest puts the package and oracle/ on the path)

import conftest  # noqa: E402,F401
import hc_prefix_support as HP  # noqa: E402
import hc_support as H  # noqa: E402
import opt_support as P  # noqa: E402

CAP_MAX_INPUT = 70000
CAP_LEVELS = {"hc": 4, "prefix": 4, "opt": 3}


def _entry(cases, compress) -> dict:
    """cases: (name, args); compress(*args) -> bytes."""
    sha = hashlib.sha256()
    names, sizes = [], []
    for name, args in cases:
        out = compress(*args)
        names.append(name)
        sizes.append(len(out))
        sha.update(len(out).to_bytes(4, "little") + out)
    return {"cases": names, "sizes": sizes, "sha256": sha.hexdigest()}


def _plain_families() -> dict:
    """family -> [(name, (data,))] of the inputs without a prefix."""
    fam = {"validity": [(name, (d,)) for name, d in H.validity_inputs()],
           "window": [(f"window-{p}", (d,)) for p, d in H.window_inputs()]}
    for kind in P.ALL_KINDS:
        fam[f"kind-{kind}"] = [(f"{kind}-{i}", (b,)) for i, b in enumerate(H.kind_blocks(kind))]
    return fam


def _short(cases) -> list:
    return [(name, args) for name, args in cases if len(args[-1]) <= CAP_MAX_INPUT]


def _split(cases) -> list:
    """Every input cut in two: its first half (at most 64 KiB) as the prefix of the rest."""
    out = []
    for name, (d,) in cases:
        cut = min(len(d) // 2, HP.PREFIX_MAX)
        out.append((name, (d[:cut], d[cut:])))
    return out


def capacity(cases, compress, level: int) -> dict:
    """The full-bound outputs' entry, whether cap = size reproduces them, and
    the results (0: refused) at cap = size - 1 and cap = 0."""
    full = [compress(*args, level, None) for _, args in cases]
    entry = _entry([(name, (out,)) for (name, _), out in zip(cases, full)], lambda out: out)
    entry["level"] = level
    entry["same_at_size"] = [compress(*args, level, len(out)) == out for (_, args), out in zip(cases, full)]
    entry["at_size_minus_1"] = [len(compress(*args, level, len(out) - 1) or b"") for (_, args), out in zip(cases, full)]
    entry["at_zero"] = [len(compress(*args, level, 0) or b"") for _, args in cases]
    return entry


def strip_names(doc):
    """The document as the fixture holds it: without the cases' names."""
    if isinstance(doc, dict):
        return {k: strip_names(v) for k, v in doc.items() if k != "cases"}
    return doc


def compute() -> dict:
    plain = _plain_families()
    kinds = [f for f in plain if f.startswith("kind-")]
    doc = {"hc": {}, "prefix": {}, "opt": {}, "capacity": {}}

    for fam, cases in plain.items():
        doc["hc"][fam] = {str(lvl): _entry(cases, lambda d, lvl=lvl: H.model_compress(d, lvl)) for lvl in (3, 4, 9)}

    grid = [(name, (p, b)) for name, p, b in HP.grid_cases()]
    edge = [(name, pb) for name, pb in HP.edge_cases().items()]
    for fam, cases, levels in (("grid", grid, (3, 9)), ("edge", edge, (4, 9))):
        doc["prefix"][fam] = {str(lvl): _entry(cases, lambda p, b, lvl=lvl: HP.model_compress_prefix(p, b, lvl))
                              for lvl in levels}

    opt_plan = [("validity", _short(plain["validity"]), (3, 9)), ("window", plain["window"], (4,))]
    opt_plan += [(fam, plain[fam], (4, 9)) for fam in kinds]
    for fam, cases, levels in opt_plan:
        doc["opt"][fam] = {str(lvl): _entry(cases, lambda d, lvl=lvl: P.model_compress(d, lvl)) for lvl in levels}

    short = _short(plain["validity"])
    doc["capacity"]["hc"] = capacity(short, lambda d, lvl, cap: H.model_compress(d, lvl, cap), CAP_LEVELS["hc"])
    doc["capacity"]["prefix"] = capacity(_split(short), lambda p, b, lvl, cap: HP.model_compress_prefix(p, b, lvl, cap),
                                         CAP_LEVELS["prefix"])
    doc["capacity"]["opt"] = capacity(short, lambda d, lvl, cap: P.model_compress(d, lvl, cap), CAP_LEVELS["opt"])
    return doc


if __name__ == "__main__":
    doc = {"comment": "sizes and SHA-256 digests (each output preceded by its LE32 length) of the outputs of the CPU "
                      "models hc_model_compress, hc_model_compress_prefix and opt_model_compress; capacity: the prefix "
                      "model takes each input's first half (at most 64 KiB) as the prefix of the rest"}
    doc.update(compute())
    text = json.dumps(strip_names(doc), indent=1)
    text = re.sub(r"\[\s+([^\[\]{}]*?)\s+\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]", text)   # lists on one line
    with open(os.path.join(HERE, "model_digests.json"), "w") as f:
        f.write(text + "\n")
    for model in ("hc", "prefix", "opt"):
        for fam, levels in doc[model].items():
            for lvl, e in levels.items():
                print(f"{model} {fam} level {lvl}: {len(e['sizes'])} cases, {sum(e['sizes'])} bytes, {e['sha256'][:16]}")

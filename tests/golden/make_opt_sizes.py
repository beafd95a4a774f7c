"""Writes tests/golden/opt_sizes.json: per kind (hc_support.KINDS plus "runs"
and "random"), the totals of the reference's LZ4_compress_HC at levels 9, 10,
11 and 12 over hc_support.kind_blocks(kind).  Needs the reference build
(oracle/_ref); run from the repository root:
    python tests/golden/make_opt_sizes.py
tests/test_opt_model.py holds the optimal parse's model against these totals
and recomputes them wherever the reference build is present."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (conftest puts the package and oracle/ on the path)

import conftest  # noqa: E402,F401
import hc_support as H  # noqa: E402

LEVELS = (9, 10, 11, 12)
KINDS = H.KINDS + ("runs", "random")


def reference_sizes(ref_so: str) -> dict:
    ref = C.CDLL(ref_so)
    ref.LZ4_compress_HC.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    out = {}
    for kind in KINDS:
        row = {f"hc{lvl}": 0 for lvl in LEVELS}
        for b in H.kind_blocks(kind):
            dst = C.create_string_buffer(H.compress_bound(len(b)))
            for lvl in LEVELS:
                row[f"hc{lvl}"] += ref.LZ4_compress_HC(b, dst, len(b), len(dst), lvl)
        out[kind] = row
    return out


if __name__ == "__main__":
    import oracle as O
    doc = {"comment": "totals over _synth.blocks(24, kind, seed=31) of the reference lz4libs v1.9.4: "
                      "LZ4_compress_HC at levels 9, 10, 11 and 12",
           "reference": reference_sizes(O.REF_SO)}
    with open(os.path.join(HERE, "opt_sizes.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["reference"], indent=1))

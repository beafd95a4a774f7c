"""Writes tests/golden/hc_prefix_sizes.json: per kind, the size of the
reference's LZ4F_compressFrame frame (linked 64 KiB blocks, no checksums,
content size stored) at HC levels 4 and 9 over the kind's 24 blocks joined
into one input, and its payload (the frame without header, per-block size
words and end mark).  Needs the reference build (oracle/_ref); run from the
repository root:  python tests/golden/make_hc_prefix_sizes.py
tests/test_hc_prefix_model.py compares the model's linked frames with these
totals and recomputes them wherever the reference build is present."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (conftest puts the package and oracle/ on the path)

import conftest  # noqa: E402,F401
import hc_prefix_support as HP  # noqa: E402
import hc_support as H  # noqa: E402


def reference_sizes(ref) -> dict:
    out = {}
    for kind in H.KINDS:
        data = b"".join(H.kind_blocks(kind))
        nb = -(-len(data) // HP.FRAME_BLOCK)
        row = {}
        for level in (4, 9):
            frame = ref.compress_frame(data, block_size_id=4, linked=True, content_checksum=False, level=level)
            row[f"frame{level}"] = len(frame)
            row[f"payload{level}"] = len(frame) - HP.FRAME_OVERHEAD - 4 * nb
        out[kind] = row
    return out


if __name__ == "__main__":
    import oracle as O
    doc = {"comment": "reference lz4libs v1.9.4: LZ4F_compressFrame(blockSizeID 4, linked, no checksums, content "
                      "size stored, compressionLevel 4 / 9) over b''.join(_synth.blocks(24, kind, seed=31)); "
                      "payload = frame - 19 - 4 * 24",
           "reference": reference_sizes(O.Reference())}
    with open(os.path.join(HERE, "hc_prefix_sizes.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["reference"], indent=1))

"""Writes tests/golden/frame_digests.json: the output bytes of the frame and
block compression calls, pinned as sizes and SHA-256 digests.  Per case: the
output sizes in order (-1: no output) and one SHA-256 over the outputs, each
preceded by its LE64 length.  The cases are the smallest shapes that take every
branch of the launch selection: every parse, linked and independent blocks,
with and without checksums and a stored size, block-size ids 0, 5 and 7, a
batch that mixes 64 KiB-block and 4 MiB-block frames, batches that mix linked
and unlinked frames (the five sizes at ids 0 and 5), and the block calls with
every table, parse and kind of dictionary.

It uses the public calls only and inputs of lz4/_synth.py, so the same file
runs on any commit: run it on the commit whose bytes are to be pinned, on an
MI355X, from the repository root:
    python tests/golden/make_frame_digests.py
It runs every case twice and refuses to write a case of the exact, HC or
optimal parses whose two runs differ; a parallel-parse case that differs is
pinned by its sizes (when those agree) and a decode round trip instead.
tests/test_gpu_frame_digests.py recomputes all of it and compares."""
import hashlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (conftest puts the package on the path)

import conftest  # noqa: E402,F401
import numpy as np  # noqa: E402

FRAME_SIZES = (0, 1, 65536, 65537, 3 * 65536 + 5)
BIG = (4 << 20) + 1
BLOCK_SIZES = (0, 13, 4096, 65536)
DICT_BYTES = 70000
# (name, parse, compression_level)
PARSES = (("exact", "exact", 0), ("parallel", "parallel", 0), ("hc4", "hc", 4), ("hc9", "hc", 9),
          ("optimal9", "optimal", 9))


def _inputs():
    from lz4 import _synth
    stream = _synth.blocks(4, "silesia", seed=31).tobytes()
    frames = [stream[100 * i: 100 * i + n] for i, n in enumerate(FRAME_SIZES)]
    big = _synth.blocks(BIG // 65536 + 1, "silesia", seed=32).tobytes()[:BIG]
    bstream = _synth.blocks(2, "text", seed=33).tobytes()
    blocks = [bstream[7 * i: 7 * i + n] for i, n in enumerate(BLOCK_SIZES)]
    dictionary = _synth.blocks(2, "text", seed=33).tobytes()[30000: 30000 + DICT_BYTES]
    return frames, big, blocks, dictionary


def _entry(outs, decodes=None) -> dict:
    sha = hashlib.sha256()
    for o in outs:
        if o is not None:
            sha.update(len(o).to_bytes(8, "little") + o)
        else:
            sha.update(b"\xff" * 8)
    e = {"sizes": [-1 if o is None else len(o) for o in outs], "sha256": sha.hexdigest()}
    if decodes is not None:
        e["decodes"] = bool(decodes)
    return e


def _pack(dev, items):
    import torch
    lens = [len(x) for x in items]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    buf = torch.frombuffer(bytearray(b"".join(items) or b"\0"), dtype=torch.uint8).to(dev)
    if not sum(lens):
        buf = buf[:0]
    return buf, torch.tensor(offs, dtype=torch.int64, device=dev), torch.tensor(lens, dtype=torch.int64, device=dev)


def _cut(buf, off, length):
    h = buf.cpu().numpy()
    return [h[o:o + n].tobytes() for o, n in zip(off.cpu().tolist(), length.cpu().tolist())]


def _frame_cases(dev, frames, big):
    """name -> (callable giving the list of frames, the inputs, whether the parse is the parallel one)."""
    import torch
    import lz4.frame as F

    def device_singles(items, **kw):
        out = []
        for d in items:
            t = torch.frombuffer(bytearray(d or b"\0"), dtype=torch.uint8).to(dev)
            out.append(F.compress_device(t, len(d), **kw).cpu().numpy().tobytes())
        return out

    def batch(items, **kw):
        return _cut(*F.compress_batch(*_pack(dev, items), **kw))

    cases = {}

    def add(tag, items, kw, parallel):
        cases[f"compress_device {tag}"] = (lambda: device_singles(items, **kw), items, parallel)
        cases[f"compress_batch {tag}"] = (lambda: batch(items, **kw), items, parallel)

    flags = list(itertools.product((True, False), (False, True), (True, False)))   # linked, checksums, store_size
    for (pname, parse, level), bs, (linked, sums, ss) in itertools.product(PARSES, (0, 5), flags):
        if parse == "optimal" and linked:
            continue
        kw = dict(parse=parse, compression_level=level, block_size=bs, block_linked=linked, content_checksum=sums,
                  block_checksum=sums, store_size=ss)
        add(f"{pname} bs{bs} {'L' if linked else '-'}{'C' if sums else '-'}{'S' if ss else '-'}", frames, kw,
            parse == "parallel")
    # block-size id 7: the large-block launch, and in the batch the split by block size (ids 4, 5 and 7 together)
    for linked, sums, ss in flags:
        kw = dict(parse="parallel", block_size=7, block_linked=linked, content_checksum=sums, block_checksum=sums,
                  store_size=ss)
        tag = f"parallel bs7 {'L' if linked else '-'}{'C' if sums else '-'}{'S' if ss else '-'}"
        cases[f"compress_device {tag}"] = (lambda kw=kw: device_singles([big], **kw), [big], True)
        mixed = frames[:3] + [big] + frames[3:]
        cases[f"compress_batch {tag} mixed"] = (lambda kw=kw, mixed=mixed: batch(mixed, **kw), mixed, True)
    cases["compress default"] = (lambda: [F.compress(d) for d in frames], frames, False)
    cases["compress_many default"] = (lambda: F.compress_many(frames), frames, False)
    return cases


def _block_cases(dev, blocks, dictionary):
    """name -> (callable giving the list of blocks (None: no output), check of a decode or None)."""
    import torch
    import lz4.block as B
    from lz4 import _native as N

    def many(**kw):
        return lambda: B.compress_many(blocks, **kw)

    def batch(items=blocks, lead=b"", **kw):
        def run():
            packed = [lead + b for b in items]
            buf, off, ln = _pack(dev, packed)
            if "dict_len" in kw:
                kw["dict_len"] = kw["dict_len"].to(dev)
            dst, dst_off, out_len = B.compress_batch(buf, off + len(lead), (ln - len(lead)).to(torch.int32), **kw)
            torch.cuda.synchronize()
            return [o if o else None for o in _cut(dst, dst_off, out_len.to(torch.int64).clamp(min=0))]
        return run

    def decode_many(outs, **kw):
        return B.decompress_many([o for o in outs], **kw) == blocks

    def decode_raw(outs, **kw):
        got = B.decompress_many([o or b"" for o in outs], uncompressed_size=[len(b) for b in blocks],
                                raise_errors=False, **kw)
        return all(o is None or g == b for o, g, b in zip(outs, got, blocks))

    n = len(blocks)
    tail = dictionary[-65536:]
    hist = torch.full((n,), len(dictionary), dtype=torch.int32)
    cases = {}
    for name, const, label in (("block", N.TABLE_U32_HASH5, "block"), ("default", N.TABLE_AUTO, "default"),
                               ("u16", N.TABLE_U16_HASH4, "u16")):
        cases[f"compress_many table={name}"] = (many(table=const), None)
        cases[f"compress_batch table={name}"] = (batch(table=label), None)
    for name, const in (("PARSE_PARALLEL", N.PARSE_PARALLEL), ("PARSE_PARALLEL_HQ", N.PARSE_PARALLEL_HQ)):
        cases[f"compress_many table={name}"] = (many(table=const), decode_many)
        cases[f"compress_batch table={name}"] = (batch(table=const), decode_raw)
    for level in (4, 9):
        hc = dict(mode="high_compression", compression=level)
        cases[f"compress_many hc{level}"] = (many(**hc), None)
        cases[f"compress_batch hc{level}"] = (batch(**hc), None)
        cases[f"compress_many hc{level} dict"] = (many(dict=dictionary, **hc), None)
        cases[f"compress_batch hc{level} dict_len"] = (batch(lead=tail, dict_len=hist, **hc), None)
    cases["compress_many optimal9"] = (many(mode="optimal", compression=9), None)
    cases["compress_batch optimal9"] = (batch(mode="optimal", compression=9), None)
    cases["compress_many dict"] = (many(dict=dictionary), None)
    cases["compress_many dict_prefix"] = (many(dict=dictionary, dict_prefix=True), None)
    prepared = B.prepare_dict(dictionary)
    cases["compress_many PARSE_PARALLEL PreparedDict"] = (
        many(table=N.PARSE_PARALLEL, dict=prepared), lambda o: decode_many(o, dict=dictionary))
    cases["compress_batch PARSE_PARALLEL PreparedDict"] = (
        batch(table=N.PARSE_PARALLEL, dict_buf=prepared), lambda o: decode_raw(o, dict=dictionary))
    return cases


def compute(only=None) -> dict:
    """{"frame": {case: entry}, "block": {case: entry}} of this tree on the current device (of the cases whose
    name only(group, name) accepts); parallel-parse entries carry "decodes": whether the outputs decode to the
    inputs."""
    import torch
    import lz4.frame as F
    dev = torch.device("cuda", 0)
    frames, big, blocks, dictionary = _inputs()
    doc = {"frame": {}, "block": {}}
    for name, (run, items, parallel) in _frame_cases(dev, frames, big).items():
        if only is not None and not only("frame", name):
            continue
        outs = run()
        doc["frame"][name] = _entry(outs, F.decompress_many(outs) == list(items) if parallel else None)
    for name, (run, decode) in _block_cases(dev, blocks, dictionary).items():
        if only is not None and not only("block", name):
            continue
        outs = run()
        doc["block"][name] = _entry(outs, decode(outs) if decode is not None else None)
    return doc


def pin(first: dict, second: dict) -> dict:
    """The fixture from two runs: a case whose runs agree keeps sizes and digest; a parallel-parse case whose runs
    differ keeps its sizes, if those agree, and the round trip; any other case that differs is an error."""
    doc = {}
    for group in first:
        doc[group] = {}
        for name, a in first[group].items():
            b = second[group][name]
            if "decodes" in a and not (a["decodes"] and b["decodes"]):
                raise SystemExit(f"{group} {name}: the output does not decode to the input")
            if a == b:
                doc[group][name] = a
            elif "decodes" in a:
                print(f"run-dependent: {group} {name}: {a['sizes']} / {b['sizes']}")
                doc[group][name] = {"decodes": True}
                if a["sizes"] == b["sizes"]:
                    doc[group][name]["sizes"] = a["sizes"]
            else:
                raise SystemExit(f"{group} {name}: two runs differ; this parse must be deterministic")
    return doc


if __name__ == "__main__":
    doc = {"comment": "sizes and SHA-256 digests (each output preceded by its LE64 length) of the outputs of the frame "
                      "and block compression calls on the inputs of make_frame_digests.py, written on an MI355X; "
                      "decodes: the outputs of a parallel-parse case decode to the inputs"}
    doc.update(pin(compute(), compute()))
    lines = ['{', ' "comment": ' + json.dumps(doc["comment"]) + ',']
    for group in ("frame", "block"):   # one entry per line
        lines.append(f' "{group}": {{')
        lines += [f'  {json.dumps(name)}: {json.dumps(e)},' for name, e in doc[group].items()]
        lines[-1] = lines[-1][:-1]
        lines.append(' }' + (',' if group == "frame" else ''))
    text = "\n".join(lines + ['}'])
    json.loads(text)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "frame_digests.json")
    with open(out, "w") as f:
        f.write(text + "\n")
    for group in ("frame", "block"):
        print(f"{group}: {len(doc[group])} cases, {sum('sha256' in e for e in doc[group].values())} with a digest")

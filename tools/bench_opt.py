#!/usr/bin/env python3
"""Throughput and size of the GPU optimal parse (lz4m_compress_opt_batch) next
to the GPU hash-chain compressor (lz4m_compress_hc_batch) at the same level
and to the reference's LZ4_compress_HC(12) on 16 host threads, in one run.

Workload: ``--blocks`` (16384) x 64 KiB blocks of ``_synth.blocks(...,
"silesia")``, device-resident; levels 4 and 9.  Per level and compressor:
``--warmup`` launches, then the median of ``--reps`` (>= 5) launches timed
with device events around the C-ABI call alone (the workspace and the output
are allocated before).  Every output block is decoded on the device and
compared with its input before any number is printed.  The reference leg
compresses the same blocks once with LZ4_compress_HC at level 12
(oracle/_ref/libref_lz4.so, ctypes releases the GIL) on ``--threads`` (16)
host threads.  Prints GiB/s of input, the optimal parse's speed and size over
the HC launch of the same level and over the level-9 HC launch, and its size
over the reference's level 12; writes the record as JSON (``--out``).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-lz4_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

from bench_hc import GIB, ref_leg


def gpu_leg(dev, blocks: np.ndarray, which: str, level: int, warmup: int, reps: int) -> dict:
    """``which``: "opt" or "hc" (lz4m_compress_<which>_batch with its own workspace)."""
    import lz4.block
    from lz4 import _native as N
    n, size = blocks.shape
    src = torch.from_numpy(blocks.reshape(-1)).to(dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * size
    ln = torch.full((n,), size, dtype=torch.int32, device=dev)
    bound = N.compress_bound(size)
    cap = torch.full((n,), bound, dtype=torch.int32, device=dev)
    dst_off = torch.arange(n, dtype=torch.int64, device=dev) * bound
    dst = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    lib = N.lib()
    name = f"lz4m_compress_{which}_batch"
    work = torch.empty(int(getattr(lib, f"lz4m_compress_{which}_workspace_size")(n, size)), dtype=torch.uint8,
                       device=dev)
    sp = N.stream_ptr()
    times = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        N.check(getattr(lib, name)(N.ptr(src), N.ptr(off), N.ptr(ln), N.ptr(dst), N.ptr(dst_off), N.ptr(cap),
                                   N.ptr(out_len), n, level, N.ptr(work), work.numel(), sp), name)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        print(f"  {which} level {level} launch {i} ({'warm-up' if i < warmup else 'timed'}): {ms:.1f} ms", flush=True)
        if i >= warmup:
            times.append(ms)
    # every block decodes to its input
    assert bool((out_len > 0).all()), "a block did not compress into its bound"
    back, _, status = lz4.block.decompress_batch(dst, dst_off, out_len, ln)
    assert torch.equal(status, ln), "a block did not decode to its length"
    assert torch.equal(back[: n * size], src), "decoded bytes differ from the input"
    med = statistics.median(times)
    return {"level": level, "launch_ms": [round(t, 3) for t in times], "median_ms": round(med, 3),
            "gib_per_s": n * size / GIB / (med / 1e3), "compressed_bytes": int(out_len.to(torch.int64).sum().item()),
            "workspace_bytes": int(work.numel())}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--levels", type=int, nargs="+", default=[4, 9])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the reference leg (never the machine's CPU count)")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opt_bench.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_opt: no HIP device (this benchmark has no CPU fall-back)")
    import oracle as O
    if not os.path.exists(O.REF_SO):
        sys.exit(f"bench_opt: {O.REF_SO} is missing (the reference leg needs the reference build)")
    from lz4 import _synth
    dev = torch.device("cuda", 0)
    blocks = np.ascontiguousarray(_synth.blocks(a.blocks, "silesia", seed=a.seed))
    rec = {"workload": f"{a.blocks} x {blocks.shape[1]} B _synth.blocks(silesia, seed={a.seed})",
           "input_bytes": int(blocks.size), "device": torch.cuda.get_device_name(0), "levels": []}
    for level in a.levels:
        o = gpu_leg(dev, blocks, "opt", level, a.warmup, a.reps)
        h = gpu_leg(dev, blocks, "hc", level, a.warmup, a.reps)
        row = {"level": level, "opt": o, "hc": h, "opt_over_hc_speed": o["gib_per_s"] / h["gib_per_s"],
               "opt_over_hc_size": o["compressed_bytes"] / h["compressed_bytes"]}
        rec["levels"].append(row)
        print(f"level {level}: optimal {o['gib_per_s']:.3f} GiB/s ({o['median_ms']:.1f} ms), HC {h['gib_per_s']:.3f} "
              f"GiB/s ({h['median_ms']:.1f} ms): speed x{row['opt_over_hc_speed']:.3f}, size "
              f"{row['opt_over_hc_size']:.4f}", flush=True)
    r = ref_leg(blocks, 12, a.threads)
    rec["reference_level_12"] = r
    print(f"LZ4_compress_HC(12) on {a.threads} threads: {r['gib_per_s']:.4f} GiB/s, {r['compressed_bytes']} bytes",
          flush=True)
    hc9 = next((w["hc"] for w in rec["levels"] if w["level"] == 9), None)
    for row in rec["levels"]:
        row["opt_over_reference_12_speed"] = row["opt"]["gib_per_s"] / r["gib_per_s"]
        row["opt_over_reference_12_size"] = row["opt"]["compressed_bytes"] / r["compressed_bytes"]
        if hc9 is not None:
            row["opt_over_hc9_speed"] = row["opt"]["gib_per_s"] / hc9["gib_per_s"]
            row["opt_over_hc9_size"] = row["opt"]["compressed_bytes"] / hc9["compressed_bytes"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({"bench": "opt", "out": os.path.relpath(a.out, ROOT),
                      "levels": {str(w["level"]): {"opt_gib_s": round(w["opt"]["gib_per_s"], 3),
                                                   "hc_gib_s": round(w["hc"]["gib_per_s"], 3),
                                                   "opt_over_hc9_speed": round(w.get("opt_over_hc9_speed", 0.0), 3),
                                                   "opt_over_ref12_size": round(w["opt_over_reference_12_size"], 4)}
                                 for w in rec["levels"]}}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Throughput and size of the GPU hash-chain (HC) compressor next to the
reference's LZ4_compress_HC on 16 host threads, in one run.

Workload: ``--blocks`` (16384) x 64 KiB blocks of ``_synth.blocks(...,
"silesia")``, device-resident; levels 4 and 9.  Per level: ``--warmup``
launches, then the median of ``--reps`` (>= 5) launches timed with device
events around lz4m_compress_hc_batch alone (the workspace and the output are
allocated before).  Every output block is decoded on the device and compared
with its input before any number is printed.  The reference leg compresses
the same blocks once with LZ4_compress_HC (oracle/_ref/libref_lz4.so, ctypes
releases the GIL) on ``--threads`` (16) host threads.  Prints GiB/s of input
for both, their size ratio, and writes the record as JSON (``--out``).

``--leg frames`` (``--leg all`` runs both): the same blocks as ONE input of
1 GiB, compressed into one LZ4 frame of 64 KiB blocks by
``lz4.frame.compress_device(parse="hc")``, linked (every block with the 64 KiB
of input before it as history, one lz4m_compress_hc_dict_batch launch) and
independent.  Per level and mode: one warm-up call, then the median of
``--reps`` whole calls (header to end mark, timed with device events); the
frame is decoded on the device and compared with the input before a number is
printed.  Where the reference build is present, LZ4F_compressFrame at the
same level, linked, runs on ONE host thread (it is one serial stream) over
the first ``--ref-mib`` MiB, and the GPU's linked frame of the same slice
gives the size ratio.  Written to ``--frames-out``.
"""
import argparse
import concurrent.futures as cf
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-lz4_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np
import torch

GIB = float(1 << 30)


def gpu_leg(dev, blocks: np.ndarray, level: int, warmup: int, reps: int) -> dict:
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
    work = torch.empty(int(lib.lz4m_compress_hc_workspace_size(n, size)), dtype=torch.uint8, device=dev)
    sp = N.stream_ptr()

    def launch():
        N.check(lib.lz4m_compress_hc_batch(N.ptr(src), N.ptr(off), N.ptr(ln), N.ptr(dst), N.ptr(dst_off), N.ptr(cap),
                                           N.ptr(out_len), n, level, N.ptr(work), work.numel(), sp),
                "lz4m_compress_hc_batch")

    times = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        print(f"  level {level} launch {i} ({'warm-up' if i < warmup else 'timed'}): {ms:.1f} ms", flush=True)
        if i >= warmup:
            times.append(ms)
    # every block decodes to its input
    assert bool((out_len > 0).all()), "a block did not compress into its bound"
    back, _, status = lz4.block.decompress_batch(dst, dst_off, out_len, ln)
    assert torch.equal(status, ln), "a block did not decode to its length"
    assert torch.equal(back[: n * size], src), "decoded bytes differ from the input"
    med = statistics.median(times)
    return {"level": level, "launch_ms": [round(t, 3) for t in times], "median_ms": round(med, 3),
            "gib_per_s": n * size / GIB / (med / 1e3), "compressed_bytes": int(out_len.to(torch.int64).sum().item())}


def ref_leg(blocks: np.ndarray, level: int, threads: int) -> dict:
    import oracle as O
    ref = C.CDLL(O.REF_SO)
    ref.LZ4_compress_HC.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    ref.LZ4_compress_HC.restype = C.c_int
    n, size = blocks.shape
    bound = size + size // 255 + 16
    base = blocks.ctypes.data

    def work(lo, hi):
        dst = np.empty(bound, dtype=np.uint8)
        dp, tot = dst.ctypes.data, 0
        for i in range(lo, hi):
            tot += ref.LZ4_compress_HC(base + i * size, dp, size, bound, level)
        return tot

    cuts = [n * t // threads for t in range(threads + 1)]
    with cf.ThreadPoolExecutor(threads) as pool:
        t0 = time.perf_counter()
        total = sum(pool.map(lambda t: work(cuts[t], cuts[t + 1]), range(threads)))
        secs = time.perf_counter() - t0
    return {"level": level, "threads": threads, "seconds": round(secs, 4), "gib_per_s": n * size / GIB / secs,
            "compressed_bytes": int(total)}


def frame_leg(dev, src: torch.Tensor, level: int, linked: bool, warmup: int, reps: int) -> dict:
    import lz4.frame
    times, frame = [], None
    for i in range(warmup + reps):
        frame = None   # (one frame alive at a time)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        frame = lz4.frame.compress_device(src, parse="hc", compression_level=level, block_size=4,
                                          block_linked=linked)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        print(f"  level {level} {'linked' if linked else 'independent'} frame {i} "
              f"({'warm-up' if i < warmup else 'timed'}): {ms:.1f} ms", flush=True)
        if i >= warmup:
            times.append(ms)
    back = lz4.frame.decompress_device(frame)
    assert torch.equal(back, src), "the decoded frame differs from the input"
    med = statistics.median(times)
    return {"call_ms": [round(t, 3) for t in times], "median_ms": round(med, 3),
            "gib_per_s": src.numel() / GIB / (med / 1e3), "frame_bytes": int(frame.numel())}


def ref_frame_leg(dev, blocks: np.ndarray, src: torch.Tensor, level: int, mib: int) -> dict:
    """LZ4F_compressFrame (linked 64 KiB blocks) on one host thread over the first
    ``mib`` MiB, and the size of the GPU's linked frame of the same bytes."""
    import lz4.frame
    import oracle as O
    n = min(mib << 20, blocks.size)
    data = blocks.reshape(-1)[:n]
    ref = O.Reference()
    t0 = time.perf_counter()
    frame = ref.compress_frame(data, block_size_id=4, linked=True, content_checksum=False, level=level)
    secs = time.perf_counter() - t0
    ours = lz4.frame.compress_device(src[:n], parse="hc", compression_level=level, block_size=4, block_linked=True)
    return {"input_bytes": int(n), "threads": 1, "seconds": round(secs, 4), "gib_per_s": n / GIB / secs,
            "frame_bytes": len(frame), "gpu_frame_bytes": int(ours.numel())}


def frames_main(a, dev, blocks: np.ndarray) -> None:
    import oracle as O
    src = torch.from_numpy(blocks.reshape(-1)).to(dev)
    rec = {"workload": f"one input of {a.blocks} x {blocks.shape[1]} B _synth.blocks(silesia, seed={a.seed}), "
                       "one frame of 64 KiB blocks, lz4.frame.compress_device(parse='hc')",
           "input_bytes": int(blocks.size), "device": torch.cuda.get_device_name(0), "levels": []}
    for level in a.levels:
        lk = frame_leg(dev, src, level, True, a.warmup, a.reps)
        ind = frame_leg(dev, src, level, False, a.warmup, a.reps)
        row = {"level": level, "linked": lk, "independent": ind,
               "linked_over_independent_speed": lk["gib_per_s"] / ind["gib_per_s"],
               "linked_over_independent_size": lk["frame_bytes"] / ind["frame_bytes"]}
        line = (f"level {level} frames: linked {lk['gib_per_s']:.3f} GiB/s ({lk['median_ms']:.1f} ms), independent "
                f"{ind['gib_per_s']:.3f} GiB/s ({ind['median_ms']:.1f} ms), linked/independent speed "
                f"{row['linked_over_independent_speed']:.3f}, size {row['linked_over_independent_size']:.4f}")
        if os.path.exists(O.REF_SO):
            r = ref_frame_leg(dev, blocks, src, level, a.ref_mib)
            row["reference"] = r
            row["speed_multiple"] = lk["gib_per_s"] / r["gib_per_s"]
            row["size_ratio_gpu_over_reference"] = r["gpu_frame_bytes"] / r["frame_bytes"]
            line += (f"; LZ4F_compressFrame on 1 thread {r['gib_per_s']:.4f} GiB/s over {a.ref_mib} MiB, "
                     f"x{row['speed_multiple']:.1f}; size GPU/reference {row['size_ratio_gpu_over_reference']:.4f}")
        rec["levels"].append(row)
        print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.frames_out)), exist_ok=True)
    with open(a.frames_out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({"bench": "hc_frames", "out": os.path.relpath(a.frames_out, ROOT),
                      "levels": {str(r["level"]): {"linked_gib_s": round(r["linked"]["gib_per_s"], 3),
                                                   "independent_gib_s": round(r["independent"]["gib_per_s"], 3)}
                                 for r in rec["levels"]}}))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=16384)
    ap.add_argument("--levels", type=int, nargs="+", default=[4, 9])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the reference leg (never the machine's CPU count)")
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hc_bench.json"))
    ap.add_argument("--leg", choices=("blocks", "frames", "all"), default="blocks")
    ap.add_argument("--frames-out", default=os.path.join(ROOT, "profiles", "hc_prefix_bench.json"))
    ap.add_argument("--ref-mib", type=int, default=64, help="MiB of the input the one-thread reference frame leg takes")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_hc: no HIP device (this benchmark has no CPU fall-back)")
    import oracle as O
    if a.leg != "frames" and not os.path.exists(O.REF_SO):
        sys.exit(f"bench_hc: {O.REF_SO} is missing (the reference leg needs the reference build)")
    from lz4 import _synth
    dev = torch.device("cuda", 0)
    blocks = np.ascontiguousarray(_synth.blocks(a.blocks, "silesia", seed=a.seed))
    if a.leg != "blocks":
        frames_main(a, dev, blocks)
        if a.leg == "frames":
            return
    rec = {"workload": f"{a.blocks} x {blocks.shape[1]} B _synth.blocks(silesia, seed={a.seed})",
           "input_bytes": int(blocks.size), "device": torch.cuda.get_device_name(0), "levels": []}
    for level in a.levels:
        g = gpu_leg(dev, blocks, level, a.warmup, a.reps)
        r = ref_leg(blocks, level, a.threads)
        row = {"level": level, "gpu": g, "reference": r, "speed_multiple": g["gib_per_s"] / r["gib_per_s"],
               "size_ratio_gpu_over_reference": g["compressed_bytes"] / r["compressed_bytes"]}
        rec["levels"].append(row)
        print(f"level {level}: GPU {g['gib_per_s']:.3f} GiB/s (median of {a.reps}: {g['median_ms']:.1f} ms), "
              f"LZ4_compress_HC on {a.threads} threads {r['gib_per_s']:.3f} GiB/s, "
              f"x{row['speed_multiple']:.2f}; size GPU/reference {row['size_ratio_gpu_over_reference']:.4f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({"bench": "hc", "out": os.path.relpath(a.out, ROOT),
                      "levels": {str(r["level"]): {"gpu_gib_s": round(r["gpu"]["gib_per_s"], 3),
                                                   "ref16_gib_s": round(r["reference"]["gib_per_s"], 3)}
                                 for r in rec["levels"]}}))


if __name__ == "__main__":
    main()

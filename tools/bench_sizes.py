#!/usr/bin/env python3
"""The decoded-size pass against the decode launch, in one run.

Inputs are device-resident ``_synth.blocks(..., "silesia")`` (the seeded
Silesia substitute), compressed on the device and packed.  Every figure is the
median of ``--reps`` (5) calls after one warm-up, wall time from the call to
the end of its device work.  Before a number is printed the sizes of both
walks are compared with the blocks' true sizes and with the decoder's
statuses.

Recorded:
  batches    the size pass with each walk and the decode launch of the same
             batch with known capacities (preallocated output, no read-back):
             16 384 x 64 KiB, 262 144 x 4 KiB, 64 x 4 MiB (parallel parse);
  crossover  both walks over 64 KiB blocks at block counts around 32 768
             (counts above the 16 384 distinct blocks repeat them), and the
             smallest swept count from which the lane walk is the faster one;
  unknown    lz4.block.decompress_batch(dst_cap=None) against the same call
             with capacities (both allocate the output: one read-back each);
  frames     lz4.frame.decompress_batch(direct=True) against direct=False on
             tools/bench_frames.py's two workloads, with the peak allocated
             bytes of each (torch.cuda.max_memory_allocated).
Writes the record as JSON (``--out``).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-lz4_amd"))

import torch

GIB = float(1 << 30)
WALKS = ("lane", "wave")


def timed(fn, warmup, reps):
    """Median wall seconds of fn() + device drain over `reps` calls after `warmup`."""
    times = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if i >= warmup:
            times.append(dt)
    return statistics.median(times), times, res


def compressed(src, n, block_bytes, table):
    """n blocks of block_bytes of src, compressed and packed: (bytes, offsets int64[n], lengths int32[n])."""
    import lz4.block
    dev = src.device
    off = torch.arange(n, dtype=torch.int64, device=dev) * block_bytes
    ln = torch.full((n,), block_bytes, dtype=torch.int32, device=dev)
    dst, dst_off, out_len = lz4.block.compress_batch(src, off, ln, table=table)
    assert int((out_len <= 0).sum()) == 0, "a block did not compress"
    packed, p_off = lz4.block.compact(dst, dst_off, out_len)
    return packed, p_off[:n].contiguous(), out_len


def batch(name, comp, c_off, c_len, block_bytes, reps):
    import lz4.block
    n = c_off.numel()
    dev = comp.device
    caps = torch.full((n,), block_bytes, dtype=torch.int32, device=dev)
    d_off = torch.arange(n, dtype=torch.int64, device=dev) * block_bytes
    out = torch.empty(n * block_bytes, dtype=torch.uint8, device=dev)
    rec = {"blocks": n, "block_bytes": block_bytes, "compressed_bytes": int(c_len.sum().item())}
    d_med, d_all, (_, _, status) = timed(
        lambda: lz4.block.decompress_batch(comp, c_off, c_len, caps, dst=out, dst_off=d_off), 1, reps)
    assert torch.equal(status, caps), "a block did not decode to its size"
    rec["decode_s"], rec["decode_all_s"] = d_med, d_all
    for walk in WALKS:
        med, every, size = timed(lambda: lz4.block.decompressed_size_batch(comp, c_off, c_len, walk=walk), 1, reps)
        assert torch.equal(size, status), f"the {walk} walk's sizes differ from the decoder's statuses"
        rec[f"size_{walk}_s"], rec[f"size_{walk}_all_s"] = med, every
        rec[f"size_{walk}_over_decode"] = med / d_med
    print(f"[{name}] {n} x {block_bytes}: decode {d_med * 1e3:.3f} ms, size pass lane "
          f"{rec['size_lane_s'] * 1e3:.3f} ms, wave {rec['size_wave_s'] * 1e3:.3f} ms", flush=True)
    return rec


def crossover(comp, c_off, c_len, counts, reps):
    import lz4.block
    distinct = c_off.numel()
    rows = []
    for n in counts:
        idx = torch.arange(n, device=comp.device) % distinct
        off, ln = c_off[idx].contiguous(), c_len[idx].contiguous()
        row = {"blocks": n}
        for walk in WALKS:
            med, every, size = timed(lambda: lz4.block.decompressed_size_batch(comp, off, ln, walk=walk), 1, reps)
            assert int((size != 65536).sum()) == 0
            row[f"{walk}_s"], row[f"{walk}_all_s"] = med, every
        rows.append(row)
        print(f"[crossover] {n:7d} blocks: lane {row['lane_s'] * 1e3:.3f} ms, wave {row['wave_s'] * 1e3:.3f} ms",
              flush=True)
    faster = [r["lane_s"] <= r["wave_s"] for r in rows]
    chosen = None
    for i, r in enumerate(rows):
        if all(faster[i:]):
            chosen = r["blocks"]
            break
    return {"block_bytes": 65536, "distinct_blocks": distinct, "sweep": rows,
            "lane_faster_from": chosen,
            "note": "lane_faster_from: the smallest swept count from which the lane walk is at least as fast at "
                    "every larger swept count (null: at none)"}


def unknown(comp, c_off, c_len, block_bytes, reps):
    import lz4.block
    n = c_off.numel()
    caps = torch.full((n,), block_bytes, dtype=torch.int32, device=comp.device)
    k_med, k_all, (a, _, sa) = timed(lambda: lz4.block.decompress_batch(comp, c_off, c_len, caps), 1, reps)
    u_med, u_all, (b, _, sb) = timed(lambda: lz4.block.decompress_batch(comp, c_off, c_len), 1, reps)
    assert torch.equal(sa, sb) and torch.equal(a, b), "dst_cap=None decodes differently"
    print(f"[unknown] {n} x {block_bytes}: with capacities {k_med * 1e3:.3f} ms, dst_cap=None {u_med * 1e3:.3f} ms",
          flush=True)
    return {"blocks": n, "block_bytes": block_bytes, "with_capacities_s": k_med, "with_capacities_all_s": k_all,
            "dst_cap_none_s": u_med, "dst_cap_none_all_s": u_all, "none_over_known": u_med / k_med}


def frames(name, src, frame_bytes, reps):
    import lz4.frame
    dev = src.device
    n = src.numel() // frame_bytes
    off = torch.arange(n, dtype=torch.int64, device=dev) * frame_bytes
    ln = torch.full((n,), frame_bytes, dtype=torch.int64, device=dev)
    fr, f_off, f_len = lz4.frame.compress_batch(src, off, ln)
    rec = {"frames": n, "frame_bytes": frame_bytes}
    for direct in (False, True):
        med, every, res = timed(lambda: lz4.frame.decompress_batch(fr, f_off, f_len, direct=direct), 1, reps)
        assert int((res[3] != 0).sum()) == 0 and torch.equal(res[0], src[:n * frame_bytes]), "frames did not decode"
        del res
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = lz4.frame.decompress_batch(fr, f_off, f_len, direct=direct)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del res
        key = "direct" if direct else "slots"
        rec[f"{key}_s"], rec[f"{key}_all_s"], rec[f"{key}_peak_allocated_bytes"] = med, every, peak
    rec["direct_over_slots"] = rec["direct_s"] / rec["slots_s"]
    print(f"[frames {name}] {n} x {frame_bytes}: slots {rec['slots_s'] * 1e3:.2f} ms "
          f"(peak {rec['slots_peak_allocated_bytes'] >> 20} MiB), direct {rec['direct_s'] * 1e3:.2f} ms "
          f"(peak {rec['direct_peak_allocated_bytes'] >> 20} MiB)", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=16384, help="64 KiB blocks of input (16384 = 1 GiB)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sizes_bench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    from lz4 import _native as N
    from lz4 import _synth
    dev = N.device()
    data = _synth.blocks(args.blocks, "silesia").reshape(-1)
    src = torch.from_numpy(data).to(dev)
    nb = args.blocks
    rec = {"tool": "tools/bench_sizes.py", "device": torch.cuda.get_device_name(dev),
           "input": "_synth.blocks(n, 'silesia'), device-resident, compressed on the device and packed",
           "timing": f"wall time of the call + device drain; median of {args.reps} calls after one warm-up",
           "batches": {}}
    c64 = compressed(src, nb, 64 << 10, "default")
    rec["batches"]["64KiB"] = batch("64KiB", *c64, 64 << 10, args.reps)
    c4 = compressed(src, nb * 16, 4 << 10, "default")
    rec["batches"]["4KiB"] = batch("4KiB", *c4, 4 << 10, args.reps)
    del c4
    big = min(64, nb // 64)
    c4m = compressed(src, big, 4 << 20, N.PARSE_PARALLEL_LARGE)
    rec["batches"]["4MiB"] = batch("4MiB", *c4m, 4 << 20, args.reps)
    del c4m
    counts = [c for c in (4096, 8192, 16384, 24576, 32768, 49152, 65536, 131072) if c <= 8 * nb]
    rec["crossover"] = crossover(*c64, counts, args.reps)
    rec["unknown"] = unknown(*c64, 64 << 10, args.reps)
    del c64
    rec["frames"] = {"small": frames("small", src, 64 << 10, args.reps),
                     "linked": frames("linked", src, 256 << 10, args.reps)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

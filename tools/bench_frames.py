#!/usr/bin/env python3
"""Many LZ4 frames per call against one call per frame, in one run.

Workloads, device-resident, of ``_synth.blocks(..., "silesia")`` (the seeded
Silesia substitute): ``small`` = 16 384 frames of 64 KiB (one block each) and
``linked`` = 4 096 frames of 256 KiB (four linked 64 KiB blocks each), 1 GiB
of input either way, default frame options.

Per workload and direction: ``lz4.frame.compress_batch`` /
``decompress_batch`` over all frames, one warm-up call and then the median of
``--reps`` (5) calls, wall time from the call to the end of its device work
(the calls read totals back, so they include their host synchronisations).
Against them a Python loop of ``compress_device`` / ``decompress_device``, one
call per frame -- the only way before the batched calls -- timed the same way
on the first ``--loop-frames`` (512) frames and SCALED LINEARLY to the whole
workload, because the loop is slow; the JSON says so.  Where the reference
build is present (oracle/_ref), its LZ4F_compressFrame / LZ4F_decompress run on
ONE host thread over the same subset through oracle/oracle.py, scaled the
same way.

Before any number is printed every batched frame is decoded by
``decompress_batch`` and compared with its input, and the subset's batched
frames are compared with the loop's.  Writes the record as JSON (``--out``).
"""
import argparse
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


def workload(dev, name, data, frame_bytes, args):
    import lz4.frame
    n = data.size // frame_bytes
    src = torch.from_numpy(data).to(dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * frame_bytes
    ln = torch.full((n,), frame_bytes, dtype=torch.int64, device=dev)
    sub = min(args.loop_frames, n)
    print(f"[{name}] {n} frames of {frame_bytes} bytes", flush=True)

    c_med, c_all, (frames, f_off, f_len) = timed(lambda: lz4.frame.compress_batch(src, off, ln), 1, args.reps)
    d_med, d_all, (out, o_off, o_len, status, read) = timed(
        lambda: lz4.frame.decompress_batch(frames, f_off, f_len), 1, args.reps)
    # everything decodes to its input before a number is printed
    assert int((status != 0).sum()) == 0, "a batched frame did not decode"
    assert torch.equal(read, f_len), "bytes_read differs from the frame length"
    assert torch.equal(o_off, off) and torch.equal(o_len, ln), "decoded spans differ from the inputs'"
    assert torch.equal(out, src), "decoded bytes differ from the input"

    h_off, h_len = f_off.cpu().tolist(), f_len.cpu().tolist()

    def loop_compress():
        return [lz4.frame.compress_device(src[i * frame_bytes:(i + 1) * frame_bytes]) for i in range(sub)]

    def loop_decompress():
        return [lz4.frame.decompress_device(frames[h_off[i]:h_off[i] + h_len[i]]) for i in range(sub)]

    lc_med, lc_all, singles = timed(loop_compress, 1, args.reps)
    ld_med, ld_all, backs = timed(loop_decompress, 1, args.reps)
    for i in range(sub):
        assert torch.equal(singles[i], frames[h_off[i]:h_off[i] + h_len[i]]), f"frame {i} differs from compress_device"
        assert torch.equal(backs[i], src[i * frame_bytes:(i + 1) * frame_bytes]), f"frame {i}: decompress_device"
    scale = n / sub
    total = n * frame_bytes
    rec = {
        "frames": n, "frame_bytes": frame_bytes, "input_bytes": total,
        "compressed_bytes": int(f_len.sum().item()),
        "batch": {"compress_s": c_med, "compress_all_s": c_all, "compress_gib_per_s": total / GIB / c_med,
                  "decompress_s": d_med, "decompress_all_s": d_all, "decompress_gib_per_s": total / GIB / d_med},
        "loop": {"measured_frames": sub, "scaled_linearly_by": scale,
                 "compress_subset_s": lc_med, "compress_subset_all_s": lc_all, "compress_s_scaled": lc_med * scale,
                 "compress_gib_per_s": sub * frame_bytes / GIB / lc_med,
                 "decompress_subset_s": ld_med, "decompress_subset_all_s": ld_all,
                 "decompress_s_scaled": ld_med * scale, "decompress_gib_per_s": sub * frame_bytes / GIB / ld_med},
    }
    rec["batch_over_loop"] = {"compress": lc_med * scale / c_med, "decompress": ld_med * scale / d_med}
    ref = reference_leg(data, frame_bytes, sub, scale, [frames[h_off[i]:h_off[i] + h_len[i]].cpu().numpy().tobytes()
                                                        for i in range(sub)], args.reps)
    if ref is not None:
        rec["reference_one_thread"] = ref
    b, lp = rec["batch"], rec["loop"]
    print(f"[{name}] compress   batch {b['compress_s'] * 1e3:9.1f} ms ({b['compress_gib_per_s']:.2f} GiB/s)   "
          f"loop x{scale:g} {lp['compress_s_scaled'] * 1e3:9.1f} ms   ratio {rec['batch_over_loop']['compress']:.1f}")
    print(f"[{name}] decompress batch {b['decompress_s'] * 1e3:9.1f} ms ({b['decompress_gib_per_s']:.2f} GiB/s)   "
          f"loop x{scale:g} {lp['decompress_s_scaled'] * 1e3:9.1f} ms   ratio "
          f"{rec['batch_over_loop']['decompress']:.1f}", flush=True)
    return rec


def reference_leg(data, frame_bytes, sub, scale, gpu_frames, reps):
    """The reference's frame calls on one host thread over the subset, or None without the reference build."""
    import oracle as O
    if not os.path.exists(O.REF_SO):
        return None
    ref = O.Reference()
    inputs = [data[i * frame_bytes:(i + 1) * frame_bytes].tobytes() for i in range(sub)]
    ct, dt = [], []
    dst = np.empty(frame_bytes, dtype=np.uint8)
    for _ in range(reps):
        t0 = time.perf_counter()
        made = [ref.compress_frame(d, block_size_id=4, linked=True, content_checksum=False) for d in inputs]
        ct.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for f in made:
            ref.decompress_frame_into(f, dst)
        dt.append(time.perf_counter() - t0)
    assert made == gpu_frames, "the batched frames differ from the reference's"
    c, d = statistics.median(ct), statistics.median(dt)
    return {"measured_frames": sub, "scaled_linearly_by": scale, "compress_subset_s": c, "decompress_subset_s": d,
            "compress_s_scaled": c * scale, "decompress_s_scaled": d * scale,
            "compress_gib_per_s": sub * frame_bytes / GIB / c, "decompress_gib_per_s": sub * frame_bytes / GIB / d}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--blocks", type=int, default=16384, help="64 KiB blocks of input (16384 = 1 GiB)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-frames", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    from lz4 import _native as N
    from lz4 import _synth
    dev = N.device()
    data = _synth.blocks(args.blocks, "silesia").reshape(-1)
    rec = {"tool": "tools/bench_frames.py", "device": torch.cuda.get_device_name(dev),
           "input": "_synth.blocks(n, 'silesia'), device-resident; default frame options (linked, content size)",
           "timing": f"wall time of the call + device drain; median of {args.reps} calls after one warm-up",
           "loop_note": "the per-frame loop is measured on `measured_frames` frames and scaled linearly to the "
                        "workload (`*_s_scaled`); it was not run over all frames",
           "workloads": {}}
    rec["workloads"]["small"] = workload(dev, "small", data, 64 << 10, args)
    rec["workloads"]["linked"] = workload(dev, "linked", data, 256 << 10, args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

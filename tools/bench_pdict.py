#!/usr/bin/env python3
"""Throughput and size of the parallel parse with a shared dictionary
(lz4m_pcompress_dict_batch) next to the two paths it sits between, in one run.

Workload: ``--blocks`` (262 144) x 4 KiB device-resident blocks -- 1 GiB --
cut in equal parts from ``_synth`` text, source and markup streams, and a
64 KiB dictionary made of the heads of the same three streams (the blocks
follow them).  The record names the kernel source it ran (sha256 of
lz4m_pcompress.hip).  Legs:

  a  lz4m_pcompress_dict_batch on the blocks as they lie, the dictionary
     stored once; lz4m_pcompress_dict_prepare timed on its own;
  b  lz4m_compress_dict_batch (the exact dictionary parse) on the same
     blocks in its staged layout, the dictionary's 64 KiB in front of every
     block: the path of ``compress_many(dict=)`` with the default table;
  c  lz4m_compress_batch with LZ4M_PARSE_PARALLEL on the same blocks, no
     dictionary: the ceiling.

Per leg: one warm-up launch, then the median of ``--reps`` (>= 5) launches
timed with device events around the launch alone (buffers allocated before).
Every output of every leg is decoded on the device (a and b with the
dictionary) and compared with the input before a number is printed.  Rates are
GiB/s of block bytes.  Where oracle/_ref is present, the reference's
LZ4_loadDict + LZ4_compress_fast_continue per block on ONE host thread over the
first ``--ref-mib`` (16) MiB, labelled as such.  Prints a/b and a/c and the
three compressed totals, writes the record as JSON (``--out``).
"""
import argparse
import concurrent.futures as cf
import ctypes as C
import hashlib
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
BLOCK = 4096
WINDOW = 65536
KINDS = ("text", "source", "markup")


def workload(n_blocks: int, seed: int):
    """(blocks uint8[n, 4096], dictionary bytes): one stream per kind; its
    head is the kind's part of the dictionary and the blocks follow it, so the
    dictionary has the blocks' vocabulary, as a trained one has."""
    from lz4 import _synth
    k3 = len(KINDS)
    per = [(n_blocks * (k + 1)) // k3 - (n_blocks * k) // k3 for k in range(k3)]
    head = [(WINDOW * (k + 1)) // k3 - (WINDOW * k) // k3 for k in range(k3)]
    with cf.ThreadPoolExecutor(k3) as pool:
        streams = list(pool.map(lambda a: _synth.KINDS[a[0]](np.random.default_rng(seed + a[1]), a[2]),
                                [(k, i, head[i] + per[i] * BLOCK) for i, k in enumerate(KINDS)]))
    blocks = np.ascontiguousarray(np.concatenate([s[h:] for s, h in zip(streams, head)]).reshape(n_blocks, BLOCK))
    return blocks, np.concatenate([s[:h] for s, h in zip(streams, head)]).tobytes()


def timed(name: str, launch, warmup: int, reps: int) -> list:
    times = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        print(f"  {name} launch {i} ({'warm-up' if i < warmup else 'timed'}): {ms:.3f} ms", flush=True)
        if i >= warmup:
            times.append(ms)
    return times


def leg_record(times, nbytes, out_len) -> dict:
    med = statistics.median(times)
    return {"launch_ms": [round(t, 3) for t in times], "median_ms": round(med, 3),
            "gib_per_s": nbytes / GIB / (med / 1e3), "compressed_bytes": int(out_len.to(torch.int64).sum().item())}


def check(dst, dst_off, out_len, ln, flat, d_dict=None) -> None:
    """Every block decodes to its input (with the dictionary when given)."""
    import lz4.block
    n = ln.numel()
    assert bool((out_len > 0).all()), "a block did not compress into its bound"
    kw = {}
    if d_dict is not None:
        kw = dict(dict_buf=d_dict, dict_off=torch.zeros(n, dtype=torch.int64, device=dst.device),
                  dict_len=torch.full((n,), d_dict.numel(), dtype=torch.int32, device=dst.device))
    back, _, status = lz4.block.decompress_batch(dst, dst_off, out_len, ln, **kw)
    assert torch.equal(status, ln), "a block did not decode to its length"
    assert torch.equal(back[: flat.numel()], flat), "decoded bytes differ from the input"


def reference_leg(blocks: np.ndarray, D: bytes, mib: int) -> dict:
    import oracle as O
    ref = C.CDLL(O.REF_SO)
    ref.LZ4_sizeofState.restype = C.c_int
    ref.LZ4_loadDict.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    ref.LZ4_resetStream.argtypes = [C.c_void_p]
    ref.LZ4_compress_fast_continue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    ref.LZ4_compress_fast_continue.restype = C.c_int
    n = min(blocks.shape[0], (mib << 20) // BLOCK)
    state = C.create_string_buffer(int(ref.LZ4_sizeofState()))
    dbuf = C.create_string_buffer(D, len(D))
    bound = BLOCK + BLOCK // 255 + 16
    dst = np.empty(bound, dtype=np.uint8)
    base, dp, total = blocks.ctypes.data, dst.ctypes.data, 0
    t0 = time.perf_counter()
    for i in range(n):   # lz4.block.compress(dict=): _block.c:93-107
        ref.LZ4_resetStream(state)
        ref.LZ4_loadDict(state, dbuf, len(D))
        total += ref.LZ4_compress_fast_continue(state, base + i * BLOCK, dp, BLOCK, bound, 1)
    secs = time.perf_counter() - t0
    return {"what": "LZ4_loadDict + LZ4_compress_fast_continue per block, one host thread", "threads": 1, "blocks": n,
            "input_bytes": n * BLOCK, "seconds": round(secs, 4), "gib_per_s": n * BLOCK / GIB / secs,
            "compressed_bytes": int(total)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=262144)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--ref-mib", type=int, default=16, help="MiB of the blocks the one-thread reference leg takes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdict_bench.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_pdict: no HIP device (this benchmark has no CPU fall-back)")
    import oracle as O
    from lz4 import _native as N
    dev = torch.device("cuda", 0)
    lib = N.lib()
    blocks, D = workload(a.blocks, a.seed)
    n, nbytes = a.blocks, a.blocks * BLOCK
    flat = torch.from_numpy(blocks.reshape(-1)).to(dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * BLOCK
    ln = torch.full((n,), BLOCK, dtype=torch.int32, device=dev)
    bound = N.compress_bound(BLOCK)
    cap = torch.full((n,), bound, dtype=torch.int32, device=dev)
    dst_off = torch.arange(n, dtype=torch.int64, device=dev) * bound
    dst = torch.empty(n * bound, dtype=torch.uint8, device=dev)
    out_len = torch.empty(n, dtype=torch.int32, device=dev)
    d_dict = N.to_device(D, dev)
    table = torch.empty(int(lib.lz4m_pcompress_dict_table_bytes()), dtype=torch.uint8, device=dev)
    sp = N.stream_ptr()
    rec = {"workload": f"{n} x {BLOCK} B blocks of _synth {'/'.join(KINDS)} (seed {a.seed}), one {len(D)} B dictionary "
                       "made of the heads of the same streams", "input_bytes": nbytes,
           "device": torch.cuda.get_device_name(0),
           "lz4m_pcompress_hip_sha256": hashlib.sha256(open(os.path.join(
               ROOT, "python-lz4_amd", "csrc", "lz4m_pcompress.hip"), "rb").read()).hexdigest()}

    # ---- a: the shared-dictionary parallel parse
    prep = timed("prepare", lambda: N.check(lib.lz4m_pcompress_dict_prepare(N.ptr(d_dict), len(D), N.ptr(table),
                                                                             table.numel(), sp), "prepare"),
                 a.warmup, a.reps)
    ta = timed("a pcompress_dict", lambda: N.check(lib.lz4m_pcompress_dict_batch(
        N.ptr(flat), N.ptr(off), N.ptr(ln), N.ptr(d_dict), len(D), N.ptr(table), N.ptr(dst), N.ptr(dst_off), N.ptr(cap),
        N.ptr(out_len), n, sp), "lz4m_pcompress_dict_batch"), a.warmup, a.reps)
    check(dst, dst_off, out_len, ln, flat, d_dict)
    rec["a_pcompress_dict"] = leg_record(ta, nbytes, out_len)
    rec["a_prepare_ms"] = {"launch_ms": [round(t, 4) for t in prep], "median_ms": round(statistics.median(prep), 4)}

    # ---- c: the parallel parse without a dictionary
    tc = timed("c parse_parallel", lambda: N.check(lib.lz4m_compress_batch(
        N.ptr(flat), N.ptr(off), N.ptr(ln), N.ptr(dst), N.ptr(dst_off), N.ptr(cap), N.ptr(out_len), n,
        N.PARSE_PARALLEL, 1, sp), "lz4m_compress_batch"), a.warmup, a.reps)
    check(dst, dst_off, out_len, ln, flat)
    rec["c_parse_parallel"] = leg_record(tc, nbytes, out_len)

    # ---- b: the exact dictionary parse on the staged layout (the dictionary before every block)
    slot = WINDOW + BLOCK
    staged = torch.empty((n, slot), dtype=torch.uint8, device=dev)
    staged[:, :WINDOW] = d_dict
    staged[:, WINDOW:] = flat.view(n, BLOCK)
    s_off = torch.arange(n, dtype=torch.int64, device=dev) * slot + WINDOW
    dlen = torch.full((n,), len(D), dtype=torch.int32, device=dev)
    tb = timed("b compress_dict", lambda: N.check(lib.lz4m_compress_dict_batch(
        N.ptr(staged), N.ptr(s_off), N.ptr(ln), N.ptr(dlen), N.ptr(dst), N.ptr(dst_off), N.ptr(cap), N.ptr(out_len), n,
        1, sp), "lz4m_compress_dict_batch"), a.warmup, a.reps)
    check(dst, dst_off, out_len, ln, flat, d_dict)
    rec["b_compress_dict_staged"] = leg_record(tb, nbytes, out_len)
    rec["b_staged_bytes"] = int(staged.numel())
    del staged

    ga, gb, gc = (rec[k]["gib_per_s"] for k in ("a_pcompress_dict", "b_compress_dict_staged", "c_parse_parallel"))
    rec["a_over_b_speed"], rec["a_over_c_speed"] = ga / gb, ga / gc
    sa, sb, sc = (rec[k]["compressed_bytes"] for k in ("a_pcompress_dict", "b_compress_dict_staged", "c_parse_parallel"))
    rec["a_over_b_size"], rec["a_over_c_size"] = sa / sb, sa / sc
    print(f"a shared dictionary {ga:.2f} GiB/s ({rec['a_pcompress_dict']['median_ms']:.2f} ms; prepare "
          f"{rec['a_prepare_ms']['median_ms']:.3f} ms), b exact dictionary parse, staged {gb:.2f} GiB/s, "
          f"c no dictionary {gc:.2f} GiB/s: a/b x{ga / gb:.2f}, a/c x{ga / gc:.3f}; compressed bytes a {sa} b {sb} c {sc} "
          f"(a/b {sa / sb:.4f}, a/c {sa / sc:.4f})", flush=True)
    if os.path.exists(O.REF_SO):
        r = rec["reference_one_thread"] = reference_leg(blocks, D, a.ref_mib)
        sub = int(out_len[: r["blocks"]].to(torch.int64).sum().item())   # leg b's sizes of the same blocks
        print(f"reference, ONE host thread, first {r['input_bytes'] >> 20} MiB: {r['gib_per_s']:.4f} GiB/s, "
              f"{r['compressed_bytes']} bytes (exact GPU parse of the same blocks: {sub})", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({"bench": "pdict", "out": os.path.relpath(a.out, ROOT), "a_gib_s": round(ga, 2),
                      "b_gib_s": round(gb, 2), "c_gib_s": round(gc, 2), "a_over_b": round(ga / gb, 2),
                      "a_over_c": round(ga / gc, 3)}))


if __name__ == "__main__":
    main()

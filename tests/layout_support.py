"""Buffer layouts and case generators for the slot-containment tests.

include/lz4m.h promises that a batched kernel writes block i's result only
inside [dst_off[i], dst_off[i] + dst_cap[i]).  The helpers here lay slots and
sources out so that a broken promise is seen: slots in a random order with
poisoned gaps between them, sources in another order between bytes that would
hurt if they were ever parsed.  Nothing here needs a GPU to import.
"""
import random

import numpy as np

GAPS = (1, 2, 3, 5, 15, 16, 17, 63, 64, 100)
FIRSTS = (1, 13, 64)
HEAD = 64        # poison bytes before the region the first slot's position counts from
TAIL = 256       # poison bytes after the last slot: longer than any one wild store chain overshoots
SRC_FILL = 0xFF  # token 15/15 and endless length bytes if a neighbour's bytes were parsed


def plan_slots(caps, seed, first=1, gaps=GAPS):
    """Place one output slot of caps[i] bytes per block, in a seeded random
    order, a gap drawn from `gaps` before each.  The first slot placed sits
    `first` bytes past the HEAD poison bytes (HEAD is a multiple of 64, so
    `first` is the slot's residue in a buffer aligned like an allocation), and
    TAIL poison bytes follow the last.  A capacity of 0 is an empty slot that
    keeps its gaps.  Returns (dst_off int64[n], total buffer size)."""
    assert first >= 0 and min(gaps) >= 1
    rng = random.Random(seed)
    order = list(range(len(caps)))
    rng.shuffle(order)
    dst_off = np.zeros(len(caps), dtype=np.int64)
    pos = HEAD + first
    for k, i in enumerate(order):
        if k:
            pos += rng.choice(gaps)
        dst_off[i] = pos
        pos += max(int(caps[i]), 0)
    return dst_off, pos + TAIL


def plan_packed(caps):
    """The layout every other test uses: ascending, back to back, from 0."""
    c = np.maximum(np.asarray(caps, dtype=np.int64), 0)
    off = np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.int64) if len(c) else np.zeros(0, np.int64)
    return off, int(c.sum())


def plan_sources(blobs, seed, alias=None):
    """Store the blobs in a seeded random order (another one than
    plan_slots(seed) gives) with 0..3 bytes of SRC_FILL between them and 64
    before the first and after the last.  Returns (alloc, src_off): `alloc`
    is the allocation as a uint8 array, and the kernels get the view
    alloc[1:], to which src_off (int64) is relative -- the base pointer is
    one byte past an allocation's alignment.  alias: entry e reads
    blobs[alias[e]], so several entries share one src_off; default one entry
    per blob."""
    rng = random.Random(seed ^ 0x5EED5)
    order = list(range(len(blobs)))
    rng.shuffle(order)
    parts, at, pos = [bytes([SRC_FILL]) * (1 + 64)], np.zeros(len(blobs), dtype=np.int64), 64
    for k, j in enumerate(order):
        if k:
            g = rng.randrange(4)
            parts.append(bytes([SRC_FILL]) * g)
            pos += g
        at[j] = pos
        parts.append(blobs[j])
        pos += len(blobs[j])
    parts.append(bytes([SRC_FILL]) * 64)
    alloc = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    idx = np.arange(len(blobs)) if alias is None else np.asarray(alias, dtype=np.int64)
    return alloc, at[idx]


def _slot_mask(size, dst_off, caps):
    """True for every byte of a `size`-byte buffer that lies inside a slot."""
    off = np.asarray(dst_off, dtype=np.int64)
    c = np.maximum(np.asarray(caps, dtype=np.int64), 0)
    edge = np.zeros(size + 1, dtype=np.int64)
    np.add.at(edge, off, 1)
    np.add.at(edge, off + c, -1)
    return np.cumsum(edge[:-1]) > 0


def outside_slots_intact(host_buf, dst_off, caps, poison):
    """Indices of all bytes of host_buf outside every slot that differ from
    `poison` (an empty array when every kernel stayed inside its slots)."""
    host_buf = np.asarray(host_buf)
    return np.flatnonzero(~_slot_mask(host_buf.size, dst_off, caps) & (host_buf != poison))


def describe_outside(bad, dst_off, caps, limit=4):
    """For an assertion message: each changed byte's nearest slot and side."""
    off = np.asarray(dst_off, dtype=np.int64)
    end = off + np.maximum(np.asarray(caps, dtype=np.int64), 0)
    out = []
    for b in np.asarray(bad)[:limit].tolist():
        before = np.where(off > b, off - b, np.iinfo(np.int64).max)   # the byte lies before these slots
        after = np.where(end <= b, b - end + 1, np.iinfo(np.int64).max)
        i, j = int(before.argmin()), int(after.argmin())
        if before[i] <= after[j]:
            out.append(f"byte {b}: {int(before[i])} before slot {i} (off {int(off[i])}, cap {int(caps[i])})")
        else:
            out.append(f"byte {b}: {int(after[j])} after slot {j} (off {int(off[j])}, cap {int(caps[j])})")
    return f"{len(bad)} byte(s) written outside every slot; " + "; ".join(out)


def assert_outside_intact(host_buf, dst_off, caps, poison, what=""):
    bad = outside_slots_intact(host_buf, dst_off, caps, poison)
    assert bad.size == 0, (what, describe_outside(bad, dst_off, caps))


# ------------------------------------------------------------ case generators
def malformed_cases(oracle, blocks, count=3000, seed=1234):
    """Mutated and truncated blocks with capacities around the true size."""
    rng = random.Random(seed)
    cases, caps = [], []
    for _ in range(count):
        b = blocks[rng.randrange(len(blocks))]
        n = rng.choice([20, 64, 100, 300, 2000, 65536])
        off = rng.randrange(0, 65536 - n + 1)
        c = bytearray(oracle.compress(b[off:off + n]))
        for _ in range(rng.randrange(4)):
            c[rng.randrange(len(c))] = rng.randrange(256)
        if rng.random() < 0.2:
            c = c[:rng.randrange(len(c) + 1)]
        cases.append(bytes(c))
        caps.append(rng.choice([n, n, n - 1, n + 1, n + 100, max(0, n - 20), 70, 0]))
    return cases, caps


def _literal_block(payload, tok=0xF0, tail=b""):
    """One sequence whose literal is `payload` (length bytes as the format
    writes them), then `tail`: a whole-literal block when tail is empty."""
    n = len(payload) - 15
    run = b"\xff" * (n // 255) + bytes([n % 255])
    return bytes([tok]) + run + payload + tail


def _long_sequence_blocks(n, seed):
    """Blocks whose sequences do not fit the row decoder's history or its
    length bytes: literals of 200-700 bytes (compressed length >= 255, the
    parse's escape), matches of 300-6000 bytes at offsets from 1 to ~5 000
    (overlapping periodic copies and far ones), zero runs."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        b = bytearray()
        while len(b) < 65536:
            k = int(rng.integers(0, 5))
            if k == 0:
                b += rng.integers(0, 256, size=int(rng.choice([1, 14, 15, 16, 200, 270, 600, 700])), dtype=np.uint8).tobytes()
            elif k == 1 and len(b) > 16:
                per = int(rng.choice([1, 2, 3, 7, 15, 16, 17, 40, 300, 900, 1300]))
                per = min(per, len(b))
                ml = int(rng.choice([300, 1300, 2000, 6000]))
                src = bytes(b[-per:])
                b += (src * (ml // per + 1))[:ml]
            elif k == 2 and len(b) > 5000:
                off = int(rng.integers(1300, 5000))
                ml = int(rng.integers(300, 3000))
                st = len(b) - off
                for i in range(ml):
                    b.append(b[st + i])
            else:
                b += bytes(int(rng.integers(64, 4096)))
        out.append(bytes(b[:65536]))
    return out


def _offset0_block(lit, ml):
    """A block whose one match has offset 0 (LZ4_decompress_safe v1.9.4 zero-fills
    it) followed by 5 final literals."""
    seq = bytes([(len(lit) << 4) | (ml - 4)]) + lit + b"\x00\x00"
    return seq + bytes([5 << 4]) + b"tail!"


def whole_literal_cases(max_len=70_000, seed=17):
    """Whole-literal blocks of up to max_len bytes and their near misses (the
    cases of test_decompress_whole_literal_blocks): (blocks, caps, valid),
    valid = the (block, decoded size) pairs that decode at the exact capacity."""
    rng = np.random.default_rng(seed)
    cases, caps, valid = [], [], []
    for L in [15, 300, 4094, 4095, 4096, 4110, 4111, 5000, 65535, 65536, 65537]:
        if L > max_len:
            continue
        p = rng.integers(0, 256, size=L, dtype=np.uint8).tobytes()
        b = _literal_block(p)
        valid.append((b, L))
        for cap in (L, L - 1, L + 100, 64):
            cases.append(b)
            caps.append(cap)
        cases += [b[:-1], b + b"x", _literal_block(p, tok=0xFF), _literal_block(p, tail=b"\x05\x00" + b"\x50abcde"),
                  _literal_block(p, tok=0xF4, tail=b"\x05\x00" + b"\x50abcde")]
        caps += [L, L + 1, L, L + 13, L + 13]
    cases += [b"\xf0" + b"\xff" * 5000, b"\xf0" + b"\xff" * 20 + b"\x01" + b"\x00" * 13]
    caps += [70_000, 70_000]
    return cases, caps, valid


def offset0_cases(count=64):
    """The offset-0 blocks and capacities of test_decompress_large_batch_edges."""
    cases = [_offset0_block(bytes([65 + k % 26]) * (k % 13), 4 + k % 11) for k in range(count)]
    caps = [k % 13 + 4 + k % 11 + 5 + (k % 3) * 40 for k in range(count)]
    return cases, caps


# capacities tried for every valid block of `size` decoded bytes: the fast
# loop starts at a capacity of 64 in both decoders, so 63 and 64 sit on
# either side of that switch
def valid_caps(size):
    return [size, max(size - 1, 0), size + 7, 0, 1, 63, 64]


def lz4_sequence(lit, off=None, ml=0):
    """One LZ4 sequence as the format writes it: `lit` literal bytes, then a
    match of ml >= 4 bytes at `off` (none: the block's last literals)."""
    m = ml - 4 if off is not None else 0
    out = bytes([(min(len(lit), 15) << 4) | min(m, 15)])
    if len(lit) >= 15:
        out += b"\xff" * ((len(lit) - 15) // 255) + bytes([(len(lit) - 15) % 255])
    out += lit
    if off is not None:
        out += off.to_bytes(2, "little")
        if m >= 15:
            out += b"\xff" * ((m - 15) // 255) + bytes([(m - 15) % 255])
    return out


# a literal run above the decoders' wave-cooperative threshold (64 bytes) of
# every residue mod 16, short ones, and one spanning a 1 024-byte wave pass
ROOM_LITS = tuple(range(60, 100)) + (16, 17, 18, 19, 31, 32, 33, 1087, 1088, 1089, 1090, 1091)
ROOM_LIT_TAILS = ((4, 5), (4, 6), (4, 7), (4, 8), (4, 9), (4, 10), (5, 7), (6, 6), (7, 5), (4, 12))
ROOM_MATCHES = (4, 5, 6, 7, 8, 15, 16, 17, 18, 19, 20, 33, 64, 65, 66, 67, 68, 70, 79, 80, 81, 82, 83, 96, 97, 1029)
ROOM_LASTS = (5, 6, 7, 8, 9, 10, 12, 13, 16, 17)
ROOM_OFFSETS = (1, 2, 7, 8, 16, 17, 40)
ROOM_EXTRA_CAP = (0, 1, 3, 16, -1, -2, -3, -5, -8)


def room_cases():
    """Blocks built so that a copy ends at every small distance from the
    capacity: 70 literals and a match, then a literal run of ln bytes, a
    match of ml bytes and f last literals, at capacities of the decoded size
    plus ROOM_EXTRA_CAP (below the size too: the copies before the sequence
    that no longer fits are made all the same).  The decoders finish copies with 16-byte stores
    wherever `room` allows; each (length mod 16, distance to the capacity)
    pair is a different last store.  Many shapes are invalid at the exact
    capacity (a match must end 5 bytes and a non-final literal 12 bytes
    before it, lz4.c:2172-2229): the oracle's status then.
    Returns (blocks, caps)."""
    rng = np.random.default_rng(23)
    noise = rng.integers(0, 256, 2048, dtype=np.uint8).tobytes()
    head = lz4_sequence(noise[:70], 35, 4)
    shapes = [(ln, ml, f, 17) for ln in ROOM_LITS for ml, f in ROOM_LIT_TAILS]
    shapes += [(ln, ml, f, off) for ml in ROOM_MATCHES for f in ROOM_LASTS for ln in (1, 20) for off in ROOM_OFFSETS]
    cases, caps = [], []
    for ln, ml, f, off in shapes:
        b = head + lz4_sequence(noise[100:100 + ln], off, ml) + lz4_sequence(noise[1500:1500 + f])
        size = 74 + ln + ml + f
        for extra in ROOM_EXTRA_CAP:
            cases.append(b)
            caps.append(size + extra)
    return cases, caps


def stale_history_block(pos, offset):
    """A block whose first match, at output position `pos`, has an offset
    reaching before the block's start (offset > pos): `pos` literals, a
    match of 8, then 60 literals so that a capacity of 64 or more holds the
    whole (invalid) block and the decoders' fast loop takes it."""
    assert 0 <= pos < 15 + 1 and offset > pos
    lit = bytes((37 * pos + k) & 0xFF for k in range(pos))
    tok = (min(pos, 15) << 4) | 4
    ext = b"\x00" if pos == 15 else b""
    tail = bytes(range(100, 160))
    return bytes([tok]) + ext + lit + offset.to_bytes(2, "little") + _literal_block(tail)


STALE_OFFSETS = (1, 2, 16, 1000, 8191, 8192, 65535)


def stale_history_cases():
    """Every (position 0..15, offset of STALE_OFFSETS) with offset > position."""
    return [stale_history_block(p, o) for o in STALE_OFFSETS for p in range(16) if o > p]

"""No batched kernel writes outside its slot, under any buffer layout.

include/lz4m.h: block i's result lies in [dst_off[i], dst_off[i] +
dst_cap[i]).  Every hot kernel ends its copies with 16-byte "wild" stores kept
legal by a `room` term; an off-by-one there lands in a neighbour's slot, where
a packed ascending layout hides it.  Here the slots lie in a random order
between poisoned gaps (tests/layout_support.py), the sources in another order
between 0xFF bytes, and after every launch all bytes outside the slots must
still be poison.  The same cases in the packed ascending layout must give the
same statuses and bytes: a result may not depend on where a block lies.
"""
import json
import os
import struct

import numpy as np
import pytest
import torch

import layout_support as LS
from lz4 import _native as N
from lz4 import _synth

gpu_test = pytest.mark.gpu
UNSET = -77_777   # a status no decoder returns


def _t(a, dtype, dev):
    return torch.tensor(np.asarray(a), dtype=dtype, device=dev)


class Memo:
    """oracle.decompress results by (blob index, capacity[, dictionary index])."""

    def __init__(self, oracle, blobs, dicts=None):
        self.oracle, self.blobs, self.dicts, self.m = oracle, blobs, dicts, {}

    def __call__(self, j, cap, d=None):
        key = (j, cap, d)
        r = self.m.get(key)
        if r is None:
            r = self.m[key] = self.oracle.decompress(self.blobs[j], cap, dict_=None if d is None else self.dicts[d])
        return r


class Cases:
    """Entries (blob index, capacity) over a list of distinct blobs."""

    def __init__(self):
        self.blobs, self.index, self.alias, self.caps = [], {}, [], []

    def blob(self, b):
        j = self.index.get(b)
        if j is None:
            j = self.index[b] = len(self.blobs)
            self.blobs.append(b)
        return j

    def add(self, b, cap):
        self.alias.append(self.blob(b))
        self.caps.append(int(cap))

    def __len__(self):
        return len(self.caps)


@pytest.fixture(scope="module")
def corpus():
    """The corpus of tests/test_gpu_codec.py (same seeds)."""
    import random
    blocks = [b.tobytes() for b in _synth.blocks(96, "silesia", seed=11)]
    rng = random.Random(5)
    sizes = [0, 1, 4, 5, 11, 12, 13, 14, 15, 16, 17, 31, 32, 63, 64, 65, 100, 255, 256, 1000, 4095, 4096,
             65535, 65536]
    return blocks, [blocks[rng.randrange(len(blocks))][:s] for s in sizes]


def _golden_decode_vectors():
    from conftest import GOLDEN
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    arr = np.load(os.path.join(GOLDEN, "golden.npz"), allow_pickle=False)
    return [(arr[e["key"]].tobytes(), e["cap"]) for e in man["decompress"]]


def edge_cases(oracle, corpus, malformed=600):
    """The decoder case set: valid blocks at the capacities of
    LS.valid_caps, malformed, offset-0 and whole-literal blocks with their
    near misses, the golden decode vectors."""
    blocks, ragged = corpus
    cs = Cases()
    plain = ragged + blocks[:8] + LS._long_sequence_blocks(4, 41)
    for b in plain:
        c = oracle.compress(b)
        for cap in LS.valid_caps(len(b)):
            cs.add(c, cap)
    wl, wcap, valid = LS.whole_literal_cases()
    for b, cap in zip(wl, wcap):
        cs.add(b, cap)
    for b, size in valid:
        for cap in LS.valid_caps(size):
            cs.add(b, cap)
    for b, cap in zip(*LS.malformed_cases(oracle, blocks, count=malformed)):
        cs.add(b, cap)
    for b, cap in zip(*LS.offset0_cases(64)):
        cs.add(b, cap)
    for b, cap in _golden_decode_vectors():
        cs.add(b, cap)
    return cs


@pytest.fixture(scope="module")
def edges(oracle, corpus):
    cs = edge_cases(oracle, corpus)
    return cs, Memo(oracle, cs.blobs)


# ------------------------------------------------------------ the checker itself (no GPU)
def test_checker_reports_every_stray_byte(oracle, corpus):
    """outside_slots_intact on a CPU-made buffer: a dozen blocks decoded by
    the oracle into a poisoned plan_slots layout leave it empty; one changed
    byte just before a slot, just after a slot or in the tail guard is
    reported, each at its index."""
    blocks, ragged = corpus
    src = [b[:1000 + 37 * i] for i, b in enumerate(blocks[:9])] + [ragged[0], ragged[5], ragged[14]]
    caps = [len(b) + (7 if i % 3 == 0 else 0) for i, b in enumerate(src)]
    caps[-1] = 0   # an empty slot keeps its gaps
    for first in LS.FIRSTS:
        dst_off, total = LS.plan_slots(caps, seed=3, first=first)
        assert sorted(dst_off.tolist()) != dst_off.tolist()          # not monotone in the block index
        assert dst_off.min() == LS.HEAD + first and total - (dst_off + np.asarray(caps)).max() == LS.TAIL
        buf = np.full(total, 0xA5, dtype=np.uint8)
        for i, b in enumerate(src):
            st, out = oracle.decompress(oracle.compress(b), caps[i])
            if st > 0:
                buf[dst_off[i]:dst_off[i] + st] = np.frombuffer(out, dtype=np.uint8)
        assert LS.outside_slots_intact(buf, dst_off, caps, 0xA5).size == 0
        for i in (0, 4, len(src) - 1):
            for at in (int(dst_off[i]) - 1, int(dst_off[i]) + caps[i], total - 1, total - LS.TAIL, 0):
                bad = buf.copy()
                bad[at] ^= 0xFF
                got = LS.outside_slots_intact(bad, dst_off, caps, 0xA5)
                assert got.tolist() == [at], (first, i, at)
                assert f"byte {at}:" in LS.describe_outside(got, dst_off, caps)
        with pytest.raises(AssertionError, match="before slot 4"):
            bad = buf.copy()
            bad[int(dst_off[4]) - 1] = 0
            LS.assert_outside_intact(bad, dst_off, caps, 0xA5)
        with pytest.raises(AssertionError, match="after slot 4"):
            bad = buf.copy()
            bad[int(dst_off[4]) + caps[4]] = 0
            LS.assert_outside_intact(bad, dst_off, caps, 0xA5)
    # the residues of the slot starts cover 0..15, as do those of the sources
    dst_off, _ = LS.plan_slots([5] * 400, seed=1)
    assert set((dst_off % 16).tolist()) == set(range(16))
    alloc, src_off = LS.plan_sources([b"abcde"] * 40, seed=1, alias=[0, 0, 7, 39])
    assert src_off[0] == src_off[1] and alloc[0] == LS.SRC_FILL and (alloc[1:65] == LS.SRC_FILL).all()
    view = alloc[1:]
    assert all(view[o:o + 5].tobytes() == b"abcde" for o in src_off) and (alloc[-64:] == LS.SRC_FILL).all()


# ------------------------------------------------------------ decoders
def run_decode(dev, cs, decoder, scattered, poison, seed=1, first=1, dicts=None, dict_of=None):
    """One launch over the entries of `cs`; (statuses, host output, dst_off).
    dicts / dict_of: lz4m_decompress_batch_dict with entry e's dictionary
    dicts[dict_of[e]]; then also returns whether the dictionary buffer came
    back unchanged."""
    n = len(cs)
    lens = [len(cs.blobs[j]) for j in cs.alias]
    if scattered:
        alloc, src_off = LS.plan_sources(cs.blobs, seed, cs.alias)
        d_src = torch.from_numpy(alloc).to(dev)[1:]
        dst_off, total = LS.plan_slots(cs.caps, seed, first)
    else:
        alloc = np.frombuffer(b"".join(cs.blobs[j] for j in cs.alias) + b"\0", dtype=np.uint8)
        src_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        d_src = torch.from_numpy(alloc.copy()).to(dev)
        dst_off, total = LS.plan_packed(cs.caps)
    d_dst = torch.full((max(total, 1),), poison, dtype=torch.uint8, device=dev)
    st = torch.full((n,), UNSET, dtype=torch.int32, device=dev)
    kw = {}
    if dicts is not None:
        dbuf = b"\xEE" * 3 + b"".join(dicts)
        doff = np.concatenate([[3], 3 + np.cumsum([len(d) for d in dicts])[:-1]])
        d_dict = torch.from_numpy(np.frombuffer(dbuf, dtype=np.uint8).copy()).to(dev)
        kw = dict(dict_buf=d_dict, dict_off=_t(doff[dict_of], torch.int64, dev),
                  dict_len=_t([len(dicts[k]) for k in dict_of], torch.int32, dev))
    N.launch_decompress(d_src, _t(src_off, torch.int64, dev), _t(lens, torch.int32, dev), d_dst,
                        _t(dst_off, torch.int64, dev), _t(cs.caps, torch.int32, dev), st, n, decoder=decoder, **kw)
    torch.cuda.synchronize()
    res = (st.cpu().numpy(), d_dst.cpu().numpy(), dst_off)
    if dicts is not None:
        return res + (d_dict.cpu().numpy().tobytes() == dbuf,)
    return res


def check_decode(res, cs, memo, poison, what, dict_of=None):
    """Statuses and decoded bytes equal the oracle's, the guards are intact;
    returns the decoded bytes per entry."""
    st, host, dst_off = res[:3]
    got = []
    for i, s in enumerate(st.tolist()):
        want = memo(cs.alias[i], cs.caps[i], None if dict_of is None else dict_of[i])
        assert s == want[0], (what, i, s, want[0], cs.caps[i])
        o = int(dst_off[i])
        out = host[o:o + s].tobytes() if s > 0 else b""
        if s >= 0:
            assert out == want[1], (what, i, s)
        got.append(out)
    LS.assert_outside_intact(host, dst_off, cs.caps, poison, what)
    return st.tolist(), got


def contained_and_layout_free(dev, cs, memo, decoder, **kw):
    """The assertions of one decoder over one case set: both poisons in the
    scattered layout, then today's packed ascending layout."""
    dict_of = kw.get("dict_of")
    runs = []
    for k, poison in enumerate((0xA5, 0x5A)):
        res = run_decode(dev, cs, decoder, True, poison, seed=11 + k, first=LS.FIRSTS[k], **kw)
        runs.append(check_decode(res, cs, memo, poison, (decoder, hex(poison)), dict_of))
        assert kw.get("dicts") is None or res[3], "the dictionary buffer was written"
    res = run_decode(dev, cs, decoder, False, 0xA5, **kw)
    runs.append(check_decode(res, cs, memo, 0xA5, (decoder, "packed"), dict_of))
    assert runs[0] == runs[1], "the result depends on the poison"
    assert runs[0] == runs[2], "the result depends on the layout"


@gpu_test
@pytest.mark.parametrize("decoder", ["rows", "hist", "auto"])
def test_decoders_stay_in_their_slots(gpu, edges, decoder):
    """Every decoder of lz4m_decompress_batch_sel on the edge-case set
    (valid blocks at capacities true, true - 1, true + 7, 0, 1, 63, 64;
    malformed, offset-0, whole-literal, golden vectors): the oracle's
    statuses and bytes, nothing written outside a slot under either poison,
    and the same results in the packed ascending layout."""
    cs, memo = edges
    contained_and_layout_free(gpu, cs, memo, decoder)


@pytest.fixture(scope="module")
def rooms(oracle):
    cs = Cases()
    for b, cap in zip(*LS.room_cases()):
        cs.add(b, cap)
    return cs, Memo(oracle, cs.blobs)


@gpu_test
@pytest.mark.parametrize("decoder", ["rows", "hist", "auto", "dict"])
def test_decoders_last_stores_stay_in_their_slots(gpu, oracle, rooms, decoder):
    """Crafted blocks whose literal runs and matches end at every small
    distance from the capacity, for every length mod 16 on both sides of the
    wave-cooperative threshold (LS.room_cases): the last store of a copy is
    where a `room` term decides between a 16-byte store and single bytes.
    "dict": the same blocks through lz4m_decompress_batch_dict with a 16-byte
    dictionary that no offset reaches."""
    cs, memo = rooms
    if decoder == "dict":
        dicts = [bytes(range(16))]
        dict_of = np.zeros(len(cs), dtype=np.int64)
        memo = Memo(oracle, cs.blobs, dicts)
        contained_and_layout_free(gpu, cs, memo, "auto", dicts=dicts, dict_of=dict_of)
    else:
        contained_and_layout_free(gpu, cs, memo, decoder)


@gpu_test
def test_auto_large_batch_stays_in_its_slots(gpu, oracle, corpus, edges):
    """"auto" past its switch-over to the rows decoder: 33 000 blocks, every
    16th one of the edge cases (at most 64 KiB + 1 of capacity), the rest
    64-763-byte corpus pieces; same assertions."""
    blocks, _ = corpus
    ecs, _ = edges
    small = [e for e in range(len(ecs)) if ecs.caps[e] <= 65537 and len(ecs.blobs[ecs.alias[e]]) <= 70_000]
    pool = [oracle.compress(blocks[i % len(blocks)][(i * 97) % 60000:(i * 97) % 60000 + 64 + i % 700])
            for i in range(512)]
    cs = Cases()
    for i in range(33_000):
        if i % 16 == 0:
            e = small[(i // 16) % len(small)]
            cs.add(ecs.blobs[ecs.alias[e]], ecs.caps[e])
        else:
            cs.add(pool[i % 512], 64 + (i % 512) % 700)
    assert len(small) <= 33_000 // 16   # every edge case is in
    contained_and_layout_free(gpu, cs, Memo(oracle, cs.blobs), "auto")


@gpu_test
def test_dict_decoder_stays_in_its_slots(gpu, oracle, corpus):
    """lz4m_decompress_batch_dict: the crafted blocks of test_decompress_dict
    and blocks the oracle compressed against dictionaries of 16, 5 000 and
    65 536 bytes, against oracle.decompress(dict_=); guards intact, the
    dictionary buffer bit-identical afterwards."""
    blocks, ragged = corpus
    dicts = [blocks[0][:30000], blocks[1][:16], blocks[2][:5000], blocks[3]]
    cs, dict_of = Cases(), []
    for k in range(64):
        lit = bytes([65 + k % 26]) * 3
        seq = bytes([(3 << 4) | 15]) + lit + (30 + k * 100).to_bytes(2, "little") + bytes([20 + k - 19])
        cs.add(seq + bytes([5 << 4]) + b"END__", 3 + 20 + k + 5 + 10)
        dict_of.append(0)
    joined = blocks[3] + blocks[4] + blocks[2]
    for d in (1, 2, 3):
        for data in (joined[65000:65000 + 300], joined[60000:60000 + 5000], blocks[4], blocks[2][2000:40000],
                     ragged[16], ragged[12]):
            c = oracle.compress_dict(data, dicts[d])
            for cap in LS.valid_caps(len(data)):
                cs.add(c, cap)
                dict_of.append(d)
    memo = Memo(oracle, cs.blobs, dicts)
    assert any(memo(cs.alias[i], cs.caps[i], dict_of[i])[0] > 0 for i in range(64))
    contained_and_layout_free(gpu, cs, memo, "auto", dicts=dicts, dict_of=np.asarray(dict_of))


def _chains(oracle):
    """Three chains of linked 64 KiB blocks from oracle.compress_linked: one
    with a stored (raw) block and a short last block, one with a corrupt
    second block.  Per chain: (payloads, raw flags, expected statuses,
    expected bytes)."""
    text = _synth.blocks(12, "text", seed=9).tobytes()
    noise = np.random.default_rng(4).integers(0, 256, 65536, dtype=np.uint8).tobytes()
    streams = [text[:3 * 65536], text[65536:2 * 65536] + noise + text[:2 * 65536 + 1234], text[100:100 + 4 * 65536]]
    out = []
    for c, data in enumerate(streams):
        pay = oracle.compress_linked(data, 65536)
        raw = [p is None for p in pay]
        pay = [data[k * 65536:(k + 1) * 65536] if r else p for k, (p, r) in enumerate(zip(pay, raw))]
        if c == 2:
            bad = bytearray(pay[1])
            for at in (len(bad) // 3, len(bad) // 2):
                bad[at] ^= 0x5B
            pay[1] = bytes(bad)
        st, hist = [], b""
        for p, r in zip(pay, raw):
            if st and st[-1] < 0:
                st.append(-1)
                continue
            s, o = (len(p), p) if r else oracle.decompress(p, 65536, dict_=hist[-65536:] or None)
            st.append(s)
            if s > 0:
                hist += o
        out.append((pay, raw, st, hist))
    assert any(out[1][1]) and min(out[2][2]) < 0 and out[2][2][-1] == -1 and min(out[0][2] + out[1][2]) > 0
    return out


@gpu_test
@pytest.mark.parametrize("batched", [True, False], ids=["chains", "chain"])
def test_chain_decoders_stay_in_their_regions(gpu, oracle, batched):
    """lz4m_decompress_chains and lz4m_decompress_chain: each chain decodes
    into exactly count * max_block bytes between poison; bytes and statuses
    are the oracle's (LZ4_decompress_safe_usingDict over the chain's own
    output), -1 after a failure, nothing outside a chain's region changes."""
    chains = _chains(oracle)
    MB = 65536
    cs = Cases()   # one entry per block of every chain
    first, count = [], []
    for pay, raw, st, hist in chains:
        first.append(len(cs))
        count.append(len(pay))
        for p in pay:
            cs.add(p, MB)
    raws = [int(r) for _, raw, _, _ in chains for r in raw]
    want_st = [s for _, _, st, _ in chains for s in st]
    region = [c * MB for c in count]
    for k, poison in enumerate((0xA5, 0x5A)):
        alloc, src_off = LS.plan_sources(cs.blobs, 21 + k, cs.alias)
        d_src = torch.from_numpy(alloc).to(gpu)[1:]
        dst_off, total = LS.plan_slots(region, 21 + k, LS.FIRSTS[k + 1])
        dst = torch.full((total,), poison, dtype=torch.uint8, device=gpu)
        st = torch.full((len(cs),), UNSET, dtype=torch.int32, device=gpu)
        so, sl = _t(src_off, torch.int64, gpu), _t([len(cs.blobs[j]) for j in cs.alias], torch.int32, gpu)
        rf = _t(raws, torch.uint8, gpu)
        if batched:
            N.launch_decompress_chains(d_src, so, sl, rf, _t(first, torch.int64, gpu), _t(count, torch.int32, gpu),
                                       dst, _t(dst_off, torch.int64, gpu), _t([MB] * len(count), torch.int32, gpu),
                                       st, len(count))
        else:
            for f, c, o in zip(first, count, dst_off.tolist()):
                N.launch_decompress_chain(d_src, so[f:f + c], sl[f:f + c], rf[f:f + c] != 0, dst[o:], st[f:f + c], c,
                                          MB)
        torch.cuda.synchronize()
        host = dst.cpu().numpy()
        assert st.cpu().tolist() == want_st, poison
        for c, (_, _, _, hist) in enumerate(chains):
            o = int(dst_off[c])
            assert host[o:o + len(hist)].tobytes() == hist, (poison, c)
        LS.assert_outside_intact(host, dst_off, region, poison, ("chains" if batched else "chain", hex(poison)))


# ------------------------------------------------------------ hist: a wave's second block
HIST_GRID, HIST_WAVES = 65536, 4   # hist_decompress_kernel: at most 65 536 workgroups of 4 waves (lz4m_decompress.hip)


def hist_previous_block(b, n):
    """The block the wave that decodes block b of n decoded just before it,
    or None: wave w of workgroup g starts at 4 g + w and steps by
    4 * gridDim.x, with gridDim.x = min(ceil(n / 4), 65 536)."""
    stride = HIST_WAVES * min((n + HIST_WAVES - 1) // HIST_WAVES, HIST_GRID)
    return b - stride if b >= stride else None


@gpu_test
def test_hist_second_block_of_a_wave(gpu, oracle, corpus):
    """n = 4 * 65 536 + 4 101 blocks on the hist decoder: the last 4 101 are
    decoded by waves that have already decoded one block, with that block's
    bytes still in their LDS history and input window.  The cases whose
    first match reaches before the block's start (which a stale history
    would serve) each follow a wave whose first block was a full 64 KiB one;
    every status and byte equals the oracle's, and every tail entry equals
    its result when decoded alone in a batch of one.

    The 64 KiB blocks sit at stride 32 among the first 4 128 entries (not 64
    over the whole batch): only waves 0..4 100 take a second block, and the
    83 stale-history cases need 83 of them."""
    blocks, ragged = corpus
    head, tail_n = HIST_GRID * HIST_WAVES, 4101
    n = head + tail_n
    before = lambda b: hist_previous_block(b, n)   # noqa: E731
    assert before(head - 1) is None and before(head) == 0
    big = [oracle.compress(b) for b in blocks[:8] + LS._long_sequence_blocks(4, 41)]
    pool = [oracle.compress(blocks[i % len(blocks)][(i * 97) % 60000:(i * 97) % 60000 + 64 + i % 700])
            for i in range(512)]
    stale = LS.stale_history_cases()
    STEP = 32
    assert len(stale) == 83 and STEP * len(stale) <= tail_n
    cs = Cases()
    is_big = np.zeros(n, dtype=bool)
    for i in range(head):
        if i % STEP == 0 and i < STEP * 129:
            cs.add(big[(i // STEP) % len(big)], 65536)
            is_big[i] = True
        else:
            cs.add(pool[i % 512], 64 + (i % 512) % 700)
    others = list(zip(*LS.offset0_cases(64)))
    for r in ragged:
        c = oracle.compress(r)
        others += [(c, len(r)), (c, 0), (c, 63), (c, 64)]
    room = tail_n - len(stale) - len(others)
    others += list(zip(*LS.malformed_cases(oracle, blocks, count=room)))
    others = iter(others)
    stale_at = []
    for k in range(tail_n):
        if k % STEP == 0 and k // STEP < len(stale):
            cs.add(stale[k // STEP], 64 + 36 * (k // STEP % 3))   # capacities 64, 100, 136: the fast loop
            stale_at.append(head + k)
        else:
            cs.add(*next(others))
    assert len(cs) == n and next(others, None) is None
    memo = Memo(oracle, cs.blobs)
    # the arrangement: every stale-history case is the second block of a wave whose first was a 64 KiB one
    for b in stale_at:
        assert before(b) is not None and is_big[before(b)], b
        assert cs.caps[b] >= 64 and memo(cs.alias[b], cs.caps[b])[0] < 0, b
        assert memo(cs.alias[before(b)], 65536)[0] == 65536
    lens = [len(cs.blobs[j]) for j in cs.alias]
    alloc, src_off = LS.plan_sources(cs.blobs, 5, cs.alias)
    d_src = torch.from_numpy(alloc).to(gpu)[1:]
    dst_off, total = LS.plan_slots(cs.caps, 5, 13)
    so, sl = _t(src_off, torch.int64, gpu), _t(lens, torch.int32, gpu)
    do, dc = _t(dst_off, torch.int64, gpu), _t(cs.caps, torch.int32, gpu)
    d_dst = torch.full((total,), 0xA5, dtype=torch.uint8, device=gpu)
    st = torch.full((n,), UNSET, dtype=torch.int32, device=gpu)
    N.launch_decompress(d_src, so, sl, d_dst, do, dc, st, n, decoder="hist")
    # the tail again, every entry alone in a batch of one, into a second buffer
    d_one = torch.full((total,), 0xA5, dtype=torch.uint8, device=gpu)
    st_one = torch.full((n,), UNSET, dtype=torch.int32, device=gpu)
    for b in range(head, n):
        N.launch_decompress(d_src, so[b:b + 1], sl[b:b + 1], d_one, do[b:b + 1], dc[b:b + 1], st_one[b:b + 1], 1,
                            decoder="hist")
    torch.cuda.synchronize()
    res = (st.cpu().numpy(), d_dst.cpu().numpy(), dst_off)
    sts, got = check_decode(res, cs, memo, 0xA5, "hist, two blocks per wave")
    one_st, one = st_one.cpu().numpy(), d_one.cpu().numpy()
    for b in range(head, n):
        s, o = int(one_st[b]), int(dst_off[b])
        assert s == sts[b], (b, s, sts[b])
        if s > 0:
            assert one[o:o + s].tobytes() == got[b], b


# ------------------------------------------------------------ rows: the scratch ladder
def rows_wantb(src_len, cap):
    """Length bytes rows_parse_kernel asks for per block (lz4m_rows.hip:
    `wantb`): none below a capacity of 64 or for an empty input, else
    min(src_len / 3, cap / 4) + 1 rounded up to 16."""
    if cap < 64 or src_len <= 0:
        return 0
    return (min(src_len // 3, cap // 4) + 1 + 15) & ~15


@gpu_test
def test_rows_scratch_ladder(gpu, oracle, corpus):
    """lz4m_decompress_batch_sel with explicit scratch (include/lz4m.h's
    ladder): too small or misaligned -> LZ4M_EINVAL and no status written;
    one byte short of 64 + 32 n + 64 -> the hist fallback; from there on any
    size is the rows decoder's, blocks whose length bytes do not fit going
    to the finisher alone.  At every accepted size the statuses and bytes are
    the oracle's and nothing outside a slot is written; a dirty, reused
    scratch gives identical results."""
    blocks, ragged = corpus
    lib = N.lib()
    cs = Cases()
    raw = b"".join(blocks[:32])
    k = 0
    while len(cs) < 600:
        size = 1000 + (k * 131) % 2000
        piece = raw[k * 2557:k * 2557 + size]
        k += 1
        c = oracle.compress(piece)
        if len(c) >= 300:
            cs.add(c, size + (k % 3) * 5)
    assert k * 2557 + 3000 <= len(raw)
    n_long = len(cs)
    c0 = cs.blobs[0]
    for cap in (0, 1, 63, 17):
        cs.add(c0, cap)
        cs.add(oracle.compress(ragged[13]), cap)
    for cap in (100, 0, 64):
        cs.add(b"", cap)
    n = len(cs)
    lens = [len(cs.blobs[j]) for j in cs.alias]
    want = [rows_wantb(l, c) for l, c in zip(lens, cs.caps)]
    assert min(want[:n_long]) > 64 and max(want[n_long:]) == 0 and min(cs.caps[:n_long]) >= 400
    D = sum(want)
    memo = Memo(oracle, cs.blobs)
    alloc, src_off = LS.plan_sources(cs.blobs, 8, cs.alias)
    d_src = torch.from_numpy(alloc).to(gpu)[1:]
    dst_off, total = LS.plan_slots(cs.caps, 8, 64)
    so, sl = _t(src_off, torch.int64, gpu), _t(lens, torch.int32, gpu)
    do, dc = _t(dst_off, torch.int64, gpu), _t(cs.caps, torch.int32, gpu)
    fixed = 64 + 32 * n
    full = int(lib.lz4m_decompress_workspace_size(n, int(d_src.numel())))
    assert full >= fixed + 64 + D, "the documented full size holds every block's length bytes"
    work = torch.empty(full + 64, dtype=torch.uint8, device=gpu)
    assert work.data_ptr() % 8 == 0

    def launch(work_ptr, work_bytes, decoder, count=n):
        dst = torch.full((total,), 0xA5, dtype=torch.uint8, device=gpu)
        st = torch.full((n,), UNSET, dtype=torch.int32, device=gpu)
        rc = lib.lz4m_decompress_batch_sel(N.ptr(d_src), N.ptr(so), N.ptr(sl), N.ptr(dst), N.ptr(do), N.ptr(dc),
                                           N.ptr(st), count, work_ptr, work_bytes, N.DECODERS[decoder],
                                           N.stream_ptr())
        torch.cuda.synchronize()
        return rc, (st.cpu().numpy(), dst.cpu().numpy(), dst_off)

    for wp, wb, what in ((work.data_ptr(), 63, "63 bytes"), (work.data_ptr() + 4, full, "misaligned")):
        for decoder in ("rows", "hist", "auto"):
            rc, (st, host, _) = launch(wp, wb, decoder)
            assert rc == N.EINVAL, (what, decoder, rc)
            assert (st == UNSET).all() and (host == 0xA5).all(), (what, decoder)
    # lens_cap = 64 + D / 2: the first allocation fits whichever block gets it, and they cannot all fit
    half = fixed + 64 + D // 2
    assert max(want) <= 64 + D // 2 < D
    results = []
    for wb, decoder in ((fixed + 63, "rows"), (fixed + 63, "auto"), (fixed + 64, "rows"), (half, "rows"),
                        (full, "rows")):
        rc, res = launch(work.data_ptr(), wb, decoder)
        assert rc == 0, (wb - fixed, decoder, rc)
        results.append(check_decode(res, cs, memo, 0xA5, ("scratch", wb - fixed, decoder)))
    assert all(r == results[0] for r in results)
    # dirty scratch: stale records of a differently sized batch under 0xFF and under random bytes
    rnd = torch.from_numpy(np.random.default_rng(2).integers(0, 256, work.numel(), dtype=np.uint8)).to(gpu)
    for fill in (None, rnd):
        if fill is None:
            work.fill_(0xFF)
        else:
            work.copy_(fill)
        rc, res = launch(work.data_ptr(), full, "rows")
        assert rc == 0
        assert check_decode(res, cs, memo, 0xA5, "dirty scratch, first run") == results[0]
        rc, _ = launch(work.data_ptr(), full, "rows", count=137)
        assert rc == 0
        rc, res = launch(work.data_ptr(), full, "rows")
        assert rc == 0
        assert check_decode(res, cs, memo, 0xA5, "dirty scratch, stale records") == results[0]


# ------------------------------------------------------------ compressors
def run_compress(dev, blobs, alias, caps, launch, seed=1, first=1, poison=0xA5, skip=None):
    """One compression launch over entries (blobs[alias[e]], caps[e]) in the
    scattered layout; launch(d_src, src_off, src_len, d_dst, dst_off,
    dst_cap, out_len, n).  skip[e]: bytes of entry e's blob that precede the
    block (its dictionary).  Returns the per-entry bytes or None; asserts the
    guards and that the source buffer came back unchanged."""
    n = len(caps)
    skip = np.zeros(n, dtype=np.int64) if skip is None else np.asarray(skip, dtype=np.int64)
    alloc, src_off = LS.plan_sources(blobs, seed, alias)
    d_alloc = torch.from_numpy(alloc).to(dev)
    lens = np.asarray([len(blobs[j]) for j in alias], dtype=np.int64) - skip
    dst_off, total = LS.plan_slots(caps, seed, first)
    d_dst = torch.full((total,), poison, dtype=torch.uint8, device=dev)
    ol = torch.full((n,), UNSET, dtype=torch.int32, device=dev)
    launch(d_alloc[1:], _t(src_off + skip, torch.int64, dev), _t(lens, torch.int32, dev), d_dst,
           _t(dst_off, torch.int64, dev), _t(caps, torch.int32, dev), ol, n)
    torch.cuda.synchronize()
    host = d_dst.cpu().numpy()
    LS.assert_outside_intact(host, dst_off, caps, poison, "compress")
    assert (d_alloc.cpu().numpy() == alloc).all(), "the source buffer was written"
    out = []
    for i, L in enumerate(ol.cpu().tolist()):
        assert 0 <= L <= max(caps[i], 0), (i, L, caps[i])
        out.append(host[dst_off[i]:dst_off[i] + L].tobytes() if L > 0 else None)
    return out


def _plain_launch(table, accel=1, max_len=None):
    def launch(src, so, sl, dst, do, dc, ol, n):
        N.launch_compress(src, so, sl, dst, do, dc, ol, n, table, accel, max_len=max_len)
    return launch


@pytest.fixture(scope="module")
def plain_blocks(corpus):
    blocks, ragged = corpus
    noise = np.random.default_rng(3).integers(0, 256, 65536, dtype=np.uint8).tobytes()
    return ragged + blocks[:12] + [bytes(65536), b"ab" * 32768, noise]


# Blocks of plain_blocks (a 1 000-byte piece, two 64 KiB silesia blocks) that
# also get every capacity of three ranges: a literal run's last 16-byte store
# is legal or not by the distance from its start to the capacity, so each
# capacity tries the runs that end just below it
SWEPT = (19, 24, 25)


def _cap_sweep(size):
    return sorted({c for c in list(range(2, 40)) + list(range(size // 2, size // 2 + 32)) +
                   list(range(size - 48, size + 1)) if c >= 0})


@gpu_test
@pytest.mark.parametrize("table", ["TABLE_U16_HASH4", "TABLE_U32_HASH5", "TABLE_AUTO"])
def test_exact_compressor_stays_in_its_slots(gpu, oracle, plain_blocks, table):
    """lz4m_compress_batch's exact parse at capacities bound, the oracle's
    size s, s - 1, len - 1, 16, 1 and 0 (three blocks: also every capacity
    of _cap_sweep): the oracle's bytes (or None where it gives None),
    nothing written outside a slot."""
    variant = getattr(N, table)
    alias, caps = [], []
    for j, b in enumerate(plain_blocks):
        s = len(oracle.compress(b, None if table == "TABLE_AUTO" else variant))
        for cap in (N.compress_bound(len(b)), s, s - 1, max(len(b) - 1, 0), 16, 1, 0):
            alias.append(j)
            caps.append(cap)
        if j in SWEPT:
            for cap in _cap_sweep(s):
                alias.append(j)
                caps.append(cap)
    got = run_compress(gpu, plain_blocks, alias, caps, _plain_launch(variant), seed=31, first=13)
    for i, (j, cap) in enumerate(zip(alias, caps)):
        want = oracle.compress(plain_blocks[j], None if table == "TABLE_AUTO" else variant, cap=cap)
        assert got[i] == want, (i, len(plain_blocks[j]), cap, None if got[i] is None else len(got[i]))


def _valid_or_none(oracle, got, plain, cap, at_bound, what):
    if got is None:
        assert not at_bound, what
        return
    assert len(got) <= cap, what
    st, out = oracle.decompress(got, len(plain))
    assert st == len(plain) and out == plain, what


def _parallel_caps_case(gpu, oracle, src, table, max_len=None, seed=41, swept=()):
    """A parallel parse at the bound, then at its own size p, p - 1, len - 1
    and 0: None or at most cap bytes the oracle decodes exactly, never None
    at the bound, guards intact (run_compress)."""
    idx = list(range(len(src)))
    bound = [N.compress_bound(len(b)) for b in src]
    first = run_compress(gpu, src, idx, bound, _plain_launch(table, max_len=max_len), seed=seed, first=1)
    alias, caps = [], []
    for j, b in enumerate(src):
        _valid_or_none(oracle, first[j], b, bound[j], True, (table, j, "bound"))
        p = len(first[j])
        for cap in [p, p - 1, max(len(b) - 1, 0), 0] + (_cap_sweep(p) if j in swept else []):
            alias.append(j)
            caps.append(cap)
    got = run_compress(gpu, src, alias, caps, _plain_launch(table, max_len=max_len), seed=seed + 1, first=64)
    for i, (j, cap) in enumerate(zip(alias, caps)):
        _valid_or_none(oracle, got[i], src[j], cap, False, (table, j, cap))


@gpu_test
@pytest.mark.parametrize("table", ["PARSE_PARALLEL", "PARSE_PARALLEL_HQ"])
def test_parallel_parse_stays_in_its_slots(gpu, oracle, plain_blocks, table):
    _parallel_caps_case(gpu, oracle, plain_blocks, getattr(N, table), swept=SWEPT)


@gpu_test
@pytest.mark.parametrize("seg", [True, False], ids=["segmented", "one-wave"])
def test_large_parse_stays_in_its_slots(gpu, oracle, seg):
    """PARSE_PARALLEL_LARGE with max_len (the segmented parse and its stitch)
    and without, on blocks of 65 537, 300 001 and 2 * 262 144 + 13 bytes."""
    raw = _synth.blocks(16, "silesia", seed=41).tobytes()
    noise = np.random.default_rng(6).integers(0, 256, 65537, dtype=np.uint8).tobytes()
    src = [raw[:65537], raw[70000:70000 + 300_001], raw[400_000:400_000 + 2 * 262144 + 13], noise]
    _parallel_caps_case(gpu, oracle, src, N.PARSE_PARALLEL_LARGE, max_len=max(map(len, src)) if seg else None, seed=51,
                        swept=(0, 1))


@gpu_test
@pytest.mark.parametrize("prefix", [False, True], ids=["ext-dict", "prefix"])
def test_dict_compressors_stay_in_their_slots(gpu, oracle, corpus, prefix):
    """lz4m_compress_dict_batch / lz4m_compress_prefix_batch, the dictionary
    tail stored before each block: the oracle's bytes at the bound, None or
    those bytes at len - 1 and 16; guards intact, source buffer (with the
    dictionaries) unchanged."""
    blocks, ragged = corpus
    joined = blocks[5] + blocks[6] + blocks[7]
    blobs, skip, dlen, alias, caps, want = [], [], [], [], [], []
    for dl in (16, 5000, 65536, 70000):
        for size in (0, 1, 13, 300, 5000, 65536):
            dic, data = joined[:dl], joined[dl:dl + size]
            tail = dic[-65536:]
            w = oracle.compress_dict(data, dic, prefix=prefix)
            assert w is not None
            blobs.append(tail + data)
            for cap in (N.compress_bound(size), max(size - 1, 0), 16):
                alias.append(len(blobs) - 1)
                skip.append(len(tail))
                dlen.append(dl)
                caps.append(cap)
                want.append(w)

    def launch(src, so, sl, dst, do, dc, ol, n):
        N.launch_compress_dict(src, so, sl, _t(dlen, torch.int32, gpu), dst, do, dc, ol, n, 1, prefix=prefix)
    got = run_compress(gpu, blobs, alias, caps, launch, seed=61, first=13, skip=skip)
    for i, cap in enumerate(caps):
        if i % 3 == 0:
            assert got[i] == want[i], (i, dlen[i], cap)
        else:
            assert got[i] is None or got[i] == want[i], (i, dlen[i], cap)


@gpu_test
@pytest.mark.parametrize("cap_kind", ["bound", "len-1", "16"])
def test_linked_compressor_stays_in_its_slots(gpu, oracle, cap_kind):
    """lz4m_compress_linked_batch, serial mode, three streams of 64 KiB
    blocks (the last one short): the oracle's linked blocks at the bound and
    at len - 1, None or those bytes at 16; guards intact."""
    text = _synth.blocks(12, "text", seed=9).tobytes()
    streams = [text[:3 * 65536], text[65536:65536 + 2 * 65536 + 777], text[5:5 + 65536]]
    blobs, alias, skip, lens, link, want = streams, [], [], [], [], []
    for s, data in enumerate(streams):
        w = oracle.compress_linked(data, 65536)
        assert None not in w
        for k in range(len(w)):
            alias.append(s)
            skip.append(k * 65536)
            lens.append(min(65536, len(data) - k * 65536))
            link.append(int(k > 0))
        want += w
    caps = [{"bound": N.compress_bound(L), "len-1": L - 1, "16": 16}[cap_kind] for L in lens]
    n = len(caps)
    alloc, src_off = LS.plan_sources(blobs, 71, alias)
    d_alloc = torch.from_numpy(alloc).to(gpu)
    dst_off, total = LS.plan_slots(caps, 71, 1)
    d_dst = torch.full((total,), 0xA5, dtype=torch.uint8, device=gpu)
    ol = torch.full((n,), UNSET, dtype=torch.int32, device=gpu)
    N.launch_compress_linked(d_alloc[1:], _t(src_off + np.asarray(skip), torch.int64, gpu), _t(lens, torch.int32, gpu),
                             _t(link, torch.int32, gpu), d_dst, _t(dst_off, torch.int64, gpu),
                             _t(caps, torch.int32, gpu), ol, n, 1, mode=N.LINKED_SERIAL)
    torch.cuda.synchronize()
    host = d_dst.cpu().numpy()
    LS.assert_outside_intact(host, dst_off, caps, 0xA5, ("linked", cap_kind))
    assert (d_alloc.cpu().numpy() == alloc).all(), "the source buffer was written"
    for i, L in enumerate(ol.cpu().tolist()):
        got = host[dst_off[i]:dst_off[i] + L].tobytes() if L > 0 else None
        if cap_kind == "16":
            assert got is None or got == want[i], i
        else:
            assert got == want[i], (i, L, len(want[i]))


# ------------------------------------------------------------ gather and frame records
@gpu_test
def test_gather_stays_in_its_slots(gpu):
    """lz4m_gather against numpy slicing: item lengths around the 16-byte
    store and the 1 024-byte wave pass, sources at any alignment, destinations
    in the scattered layout."""
    lens = [0, 1, 15, 16, 17, 1023, 1024, 1025, 70_001] * 3
    rng = np.random.default_rng(12)
    buf = rng.integers(0, 256, 400_000, dtype=np.uint8)
    src_off = rng.integers(0, len(buf) - 70_001, len(lens))
    src_off[:9] = [3, 5, 7, 16, 33, 1, 64, 127, 9]
    for k, poison in enumerate((0xA5, 0x5A)):
        dst_off, total = LS.plan_slots(lens, 81 + k, LS.FIRSTS[k])
        out = torch.full((total,), poison, dtype=torch.uint8, device=gpu)
        N.gather(torch.from_numpy(buf).to(gpu), _t(src_off, torch.int64, gpu), _t(lens, torch.int32, gpu), out,
                 _t(dst_off, torch.int64, gpu), len(lens))
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        for i, L in enumerate(lens):
            assert (host[dst_off[i]:dst_off[i] + L] == buf[src_off[i]:src_off[i] + L]).all(), (i, L)
        LS.assert_outside_intact(host, dst_off, lens, poison, "gather")


@gpu_test
@pytest.mark.parametrize("block_checksum", [False, True])
def test_frame_emit_stays_in_its_records(gpu, oracle, block_checksum):
    """lz4m_frame_block_sizes + lz4m_frame_emit: each record equals one
    built here (LE32 size with bit 31 for a stored raw block, payload, LE32
    XXH32 of the payload), around the stored-raw rule (cmp_len 0, raw_len - 1,
    raw_len, raw_len + 1; lz4frame.c:838) and the 16-byte store; nothing
    outside a record is written."""
    rng = np.random.default_rng(13)
    raw_buf = rng.integers(0, 256, 300_000, dtype=np.uint8)
    cmp_buf = rng.integers(0, 256, 300_000, dtype=np.uint8)
    raw_len, cmp_len = [], []
    for r in (1, 15, 16, 17, 18, 1000, 1024, 65536, 70_001):
        for c in (0, r - 1, r, r + 1, 1, 15, 16, 17):
            raw_len.append(r)
            cmp_len.append(c)
    n = len(raw_len)
    raw_off = rng.integers(0, len(raw_buf) - 70_002, n)
    cmp_off = rng.integers(0, len(cmp_buf) - 70_002, n)
    rl, cl = _t(raw_len, torch.int32, gpu), _t(cmp_len, torch.int32, gpu)
    rec = torch.full((n,), UNSET, dtype=torch.int32, device=gpu)
    N.frame_block_sizes(rl, cl, block_checksum, rec, n)
    want = []
    for i in range(n):
        stored = cmp_len[i] <= 0 or cmp_len[i] >= raw_len[i]
        pay = (raw_buf[raw_off[i]:raw_off[i] + raw_len[i]] if stored
               else cmp_buf[cmp_off[i]:cmp_off[i] + cmp_len[i]]).tobytes()
        w = struct.pack("<I", len(pay) | (0x80000000 if stored else 0)) + pay
        want.append(w + (struct.pack("<I", oracle.xxh32(pay)) if block_checksum else b""))
    assert rec.cpu().tolist() == [len(w) for w in want]
    sizes = [len(w) for w in want]
    frame_off, total = LS.plan_slots(sizes, 91, 13)
    frame = torch.full((total,), 0xA5, dtype=torch.uint8, device=gpu)
    N.frame_emit(torch.from_numpy(raw_buf).to(gpu), _t(raw_off, torch.int64, gpu), rl,
                 torch.from_numpy(cmp_buf).to(gpu), _t(cmp_off, torch.int64, gpu), cl, frame,
                 _t(frame_off, torch.int64, gpu), block_checksum, n)
    torch.cuda.synchronize()
    host = frame.cpu().numpy()
    for i, w in enumerate(want):
        assert host[frame_off[i]:frame_off[i] + len(w)].tobytes() == w, (i, raw_len[i], cmp_len[i])
    LS.assert_outside_intact(host, frame_off, sizes, 0xA5, "frame_emit")

"""The walk over a frame's block records has one implementation
(walk_records, lz4m_frames.hip) behind two entry points: lz4m_frame_scan (one
frame, lz4.frame.decompress_device) and lz4m_frames_scan + lz4m_frames_records
(a batch).  Hand-built frames of a few records of a few bytes each: both entry
points on the same bytes (the batch with n = 1), and lz4m_frame_scan's four
result values against literals -- the states include/lz4m.h documents."""
import struct

import pytest

pytestmark = pytest.mark.gpu

MAX_REC = 3
HSIZE = 7


def _frame(payloads, *, block_checksum=False, content_checksum=False, endmark=True):
    """Header (no content size), one record per (payload, stored), endmark, content checksum; the walk verifies no
    checksum, so their bytes are arbitrary."""
    from lz4 import _native as N
    desc = bytes([(1 << 6) | (1 << 5) | (block_checksum << 4) | (content_checksum << 2), 4 << 4])
    out = struct.pack("<I", 0x184D2204) + desc + bytes([(N.xxh32_host(desc) >> 8) & 0xFF])
    for payload, stored in payloads:
        out += struct.pack("<I", len(payload) | (0x80000000 if stored else 0)) + payload
        out += b"\xc5\xc6\xc7\xc8" if block_checksum else b""
    if endmark:
        out += struct.pack("<I", 0) + (b"\xa1\xa2\xa3\xa4" if content_checksum else b"")
    return out


A, B, C, D = (b"abc", 0), (b"\x11" * 5, 1), (b"z", 0), (b"four", 1)


def _cases():
    """(name, frame bytes, block checksums, content checksum, the literal (records, state, end, checksum position))"""
    three = _frame([A, B, C])
    too_large = bytearray(_frame([A, B]))
    struct.pack_into("<I", too_large, HSIZE + 4 + 3, 65537)            # the second record's size, above 64 KiB
    out = []
    for bc in (False, True):
        for cc in (False, True):
            f = _frame([A, B], block_checksum=bc, content_checksum=cc)
            out.append((f"complete bc={bc} cc={cc}", f, bc, cc,
                        (2, 0, len(f), len(f) - 4 if cc else -1)))
    full_cc = _frame([A, B], content_checksum=True)
    out += [
        ("no records", _frame([]), False, False, (0, 0, HSIZE + 4, -1)),
        ("truncated inside a header", three[:HSIZE + 4 + 3 + 2], False, False, (1, 1, 0, -1)),
        ("truncated inside a payload", three[:HSIZE + 4 + 3 + 4 + 2], False, False, (1, 1, 0, -1)),
        ("truncated inside a block checksum", _frame([A, B], block_checksum=True)[:HSIZE + 4 + 3 + 2], True, False,
         (0, 1, 0, -1)),
        ("missing endmark", _frame([A, B], endmark=False), False, False, (2, 1, 0, -1)),
        ("block size above the maximum", bytes(too_large), False, False, (1, 2, 0, -1)),
        ("content checksum missing", full_cc[:-4], False, True, (2, 3, 0, -1)),
        ("content checksum cut", full_cc[:-1], False, True, (2, 3, 0, -1)),
        ("exactly max_rec records", three, False, False, (MAX_REC, 0, len(three), -1)),
        ("max_rec + 1 records", _frame([A, B, C, D]), False, False, (MAX_REC, 4, 0, -1)),
        ("max_rec + 1 records, no endmark", _frame([A, B, C, D], endmark=False), False, False, (MAX_REC, 4, 0, -1)),
    ]
    return out


CASES = _cases()
# lz4m_frame_scan's state for a status of lz4m_frames_scan (LZ4M_FRAME_OK, _TRUNCATED, _BLOCK_TOO_LARGE,
# _CONTENT_CHECKSUM_MISSING)
STATE_OF_STATUS = {0: 0, 8: 1, 7: 2, 9: 3}


def _single(gpu, f, bc, cc, with_crc=True):
    import torch
    from lz4 import _native as N
    buf = torch.frombuffer(bytearray(f), dtype=torch.uint8).to(gpu)
    pos = torch.full((MAX_REC + 1,), -7, dtype=torch.int64, device=gpu)   # one guard entry past max_rec each
    ln = torch.full((MAX_REC + 1,), -7, dtype=torch.int32, device=gpu)
    raw = torch.full((MAX_REC + 1,), 0xEE, dtype=torch.uint8, device=gpu)
    crc = torch.full((MAX_REC + 1,), -7, dtype=torch.int64, device=gpu) if with_crc else None
    res = torch.zeros(4, dtype=torch.int64, device=gpu)
    N.frame_scan(buf, len(f), HSIZE, bc, cc, 65536, MAX_REC, pos, ln, raw, crc, res)
    arrays = [pos, ln, raw] + ([crc] if with_crc else [])
    return tuple(res.cpu().tolist()), [a.cpu().tolist() for a in arrays]


def _batched(gpu, f):
    import torch
    from lz4 import _native as N
    buf = torch.frombuffer(bytearray(f), dtype=torch.uint8).to(gpu)
    off = torch.zeros(1, dtype=torch.int64, device=gpu)
    ln = torch.tensor([len(f)], dtype=torch.int64, device=gpu)
    S = N.frames_scan(buf, off, ln, 1)
    nb = int(S["nblocks"][0])
    R = None
    if nb:
        base = N.exclusive_scan(S["nblocks"])
        R = N.frames_records(buf, off, ln, S, base, torch.zeros(1, dtype=torch.int64, device=gpu), 1, nb)
        R = [R[k].cpu().tolist() for k in ("pos", "len", "raw", "crc")]
    return {k: int(v[0]) for k, v in S.items()}, nb, R


@pytest.mark.parametrize("name,f,bc,cc,want", CASES, ids=[c[0] for c in CASES])
def test_frame_scan_states_and_records(gpu, name, f, bc, cc, want):
    res, arrays = _single(gpu, f, bc, cc)
    assert res == want
    k = res[0]
    for a, guard in zip(arrays, (-7, -7, 0xEE, -7)):
        assert a[k:] == [guard] * (MAX_REC + 1 - k), "a store past the records walked"
    # the records, from the construction: positions follow from the sizes
    payloads = {"no records": []}.get(name, [A, B, C, D])
    p = HSIZE
    for i in range(k):
        size, stored = len(payloads[i][0]), payloads[i][1]
        assert (arrays[0][i], arrays[1][i], arrays[2][i]) == (p + 4, size, stored)
        assert arrays[3][i] == (p + 4 + size if bc else -1)
        p += 4 + size + (4 if bc else 0)
    # without the checksum-position array: the same values
    res2, arrays2 = _single(gpu, f, bc, cc, with_crc=False)
    assert res2 == res and arrays2 == arrays[:3]


@pytest.mark.parametrize("name,f,bc,cc,want", CASES, ids=[c[0] for c in CASES])
def test_frame_scan_agrees_with_the_batched_walk(gpu, name, f, bc, cc, want):
    res, arrays = _single(gpu, f, bc, cc)
    S, nb, R = _batched(gpu, f)
    assert S["hsize"] == HSIZE and bool(S["flags"] & 2) == bc and bool(S["flags"] & 4) == cc
    if res[1] == 4:   # the batched walk has no record limit: it sees a complete frame, or its missing endmark
        assert (S["status"], nb) == ((0, MAX_REC + 1) if f.endswith(b"\0\0\0\0") else (8, 0))
        return
    assert STATE_OF_STATUS[S["status"]] == res[1]
    assert (S["end"], S["cpos"]) == (res[2], res[3])
    if res[1] == 0:
        assert nb == res[0]
        if nb:
            assert R == [a[:nb] for a in arrays]
    else:
        assert nb == 0   # a malformed frame decodes nothing

"""The two argument resolvers of block compression, as tables: the arguments of
lz4.block's compress / compress_many / compress_batch and of lz4.frame's
compress_device / compress_batch map to the parse description
(lz4._native.Parse) that the one launch function dispatches on, or to the
exception the call raised before the resolvers existed -- type and message
copied from that source.  No GPU: the resolvers look at no data."""
import pytest

import lz4.block._block as B
import lz4.frame._frame as F
from lz4 import _native as N

P = N.Parse
PD = B.PreparedDict(None, 70000, None)
D = b"d" * 100

BAD_MODE_MANY = "Invalid mode argument: {}. Must be one of: default, high_compression, optimal"
BAD_MODE_ONE = "Invalid mode argument: {}. Must be one of: standard, fast, high_compression, optimal"
OPT_DICT = ("mode='optimal' with a dictionary (dict= / dict_len=) is not built: the optimal "
            "parse has no history; use mode='high_compression' with a dictionary")
HC_DICT_ONE = ("mode='high_compression' with dict= (LZ4_loadDictHC) is not built on the MI355X codec; "
               "compress without a dictionary, or use mode='default' or mode='fast' with dict=")
PREPARED = "a PreparedDict is only valid with table=PARSE_PARALLEL, mode='default' and no dict_prefix"
BUF_HC = "dict_buf is not valid with mode='high_compression' (use dict_len)"
BUF_AND_LEN = "dict_buf (one shared dictionary) and dict_len (one per block) exclude each other"
BUF_TABLE = "dict_buf is only valid with table=PARSE_PARALLEL"
LEN_NOT_HC = "dict_len is only valid with mode='high_compression'"

# (arguments of lz4.block's resolve_parse, the description or (exception type, message))
BLOCK = [
    # compress(): single=True, the acceleration and level already C ints
    (dict(mode="default", accel=7, single=True), P("table", N.TABLE_U32_HASH5, 1)),
    (dict(mode="fast", accel=7, single=True), P("table", N.TABLE_U32_HASH5, 7)),
    (dict(mode="fast", accel=3, dict=D, single=True), P("table", N.TABLE_U32_HASH5, 3, history="hist")),
    (dict(mode="high_compression", compression=4, single=True), P("hc", level=4)),
    (dict(mode="optimal", compression=9, single=True), P("opt", level=9)),
    (dict(mode=3, single=True), (TypeError, "compress() argument 'mode' must be str, not int")),
    (dict(mode=None, single=True), (TypeError, "compress() argument 'mode' must be str, not NoneType")),
    (dict(mode="standard", single=True), (ValueError, BAD_MODE_ONE.format("standard"))),
    (dict(mode="hc", single=True), (ValueError, BAD_MODE_ONE.format("hc"))),
    (dict(mode="optimal", dict=D, single=True), (NotImplementedError, OPT_DICT)),
    (dict(mode="optimal", dict=b"", single=True), (NotImplementedError, OPT_DICT)),
    (dict(mode="high_compression", dict=D, single=True), (NotImplementedError, HC_DICT_ONE)),
    # compress_many()
    (dict(), P("table", N.TABLE_U32_HASH5, 1)),
    (dict(accel=5, table=N.TABLE_AUTO), P("table", N.TABLE_AUTO, 5)),
    (dict(table=N.TABLE_U16_HASH4), P("table", N.TABLE_U16_HASH4, 1)),
    (dict(table=N.PARSE_PARALLEL), P("table", N.PARSE_PARALLEL, 1)),
    (dict(table=N.PARSE_PARALLEL_HQ), P("table", N.PARSE_PARALLEL_HQ, 1)),
    (dict(table=N.PARSE_PARALLEL_LARGE), P("table", N.PARSE_PARALLEL_LARGE, 1)),
    (dict(dict=D, accel=2), P("table", N.TABLE_U32_HASH5, 2, history="hist")),
    (dict(dict=b""), P("table", N.TABLE_U32_HASH5, 1, history="hist")),
    (dict(dict=D, dict_prefix=True), P("table", N.TABLE_U32_HASH5, 1, history="hist", prefix=True)),
    (dict(dict=D, table=N.TABLE_AUTO), P("table", N.TABLE_U32_HASH5, 1, history="hist")),
    (dict(dict=D, table=N.PARSE_PARALLEL), P("table", N.PARSE_PARALLEL, history="shared")),
    (dict(dict=PD, table=N.PARSE_PARALLEL), P("table", N.PARSE_PARALLEL, history="shared")),
    (dict(dict=D, table=N.PARSE_PARALLEL, dict_prefix=True),
     P("table", N.TABLE_U32_HASH5, 1, history="hist", prefix=True)),
    (dict(mode="high_compression"), P("hc", level=9)),
    (dict(mode="high_compression", compression=4, accel=9, table=N.PARSE_PARALLEL), P("hc", level=4)),
    (dict(mode="high_compression", compression=0, dict=D), P("hc", level=0, history="hist")),
    (dict(mode="high_compression", dict=D, table=N.PARSE_PARALLEL), P("hc", level=9, history="hist")),
    (dict(mode="optimal", compression=12), P("opt", level=12)),
    (dict(mode="fast"), (ValueError, BAD_MODE_MANY.format("fast"))),
    (dict(mode="hc"), (ValueError, BAD_MODE_MANY.format("hc"))),
    (dict(mode=3), (ValueError, BAD_MODE_MANY.format(3))),
    (dict(mode=None), (ValueError, BAD_MODE_MANY.format(None))),
    (dict(mode="optimal", dict=D), (NotImplementedError, OPT_DICT)),
    (dict(mode="optimal", dict=PD, table=N.PARSE_PARALLEL), (NotImplementedError, OPT_DICT)),
    (dict(dict=PD), (ValueError, PREPARED)),
    (dict(dict=PD, table=N.TABLE_AUTO), (ValueError, PREPARED)),
    (dict(dict=PD, table=N.PARSE_PARALLEL, dict_prefix=True), (ValueError, PREPARED)),
    (dict(dict=PD, table=N.PARSE_PARALLEL, mode="high_compression"), (ValueError, PREPARED)),
    (dict(compression="9"), (TypeError, "'str' object cannot be interpreted as an integer")),
    (dict(mode="optimal", compression=2 ** 31), (OverflowError, "signed integer is greater than maximum")),
    # compress_batch(): table by name too, dict_len / dict_buf
    (dict(table="block", accel=1), P("table", N.TABLE_U32_HASH5, 1)),
    (dict(table="default", accel=4), P("table", N.TABLE_AUTO, 4)),
    (dict(table="u16"), P("table", N.TABLE_U16_HASH4, 1)),
    (dict(table="block", mode="high_compression", compression=4, dict_len=object()),
     P("hc", level=4, history="hist")),
    (dict(table=N.PARSE_PARALLEL, dict_buf=PD), P("table", N.PARSE_PARALLEL, history="shared")),
    (dict(table=N.PARSE_PARALLEL, dict_buf=object()), P("table", N.PARSE_PARALLEL, history="shared")),
    (dict(mode="optimal", dict_len=object()), (NotImplementedError, OPT_DICT)),
    (dict(mode="optimal", dict_buf=PD, table=N.PARSE_PARALLEL), (NotImplementedError, OPT_DICT)),
    (dict(mode="high_compression", dict_buf=PD, table=N.PARSE_PARALLEL), (ValueError, BUF_HC)),
    (dict(mode="high_compression", dict_buf=PD, dict_len=object()), (ValueError, BUF_HC)),
    (dict(dict_buf=PD, dict_len=object(), table=N.PARSE_PARALLEL), (ValueError, BUF_AND_LEN)),
    (dict(dict_buf=PD, table="block"), (ValueError, BUF_TABLE)),
    (dict(dict_buf=PD, table=N.PARSE_PARALLEL_HQ), (ValueError, BUF_TABLE)),
    (dict(dict_len=object(), table="block"), (ValueError, LEN_NOT_HC)),
    (dict(dict_len=object(), table=N.PARSE_PARALLEL), (ValueError, LEN_NOT_HC)),
    (dict(table="garbage"), (ValueError, "invalid literal for int() with base 10: 'garbage'")),
]

BAD_PARSE = "parse must be 'exact', 'parallel', 'hc' or 'optimal'"
LOW = "parse='{}' needs compression_level >= 3 (levels 0-2 are the fast compressor)"
HIGH = "LZ4 HC compression levels (>= 3) are outside the MI355X codec's scope"
LINKED_OPT = ("parse='optimal' has no history: block_linked=True is not built "
              "(pass block_linked=False, or parse='hc' for linked blocks)")

# ((parse, compression_level, block_linked), the description or (exception type, message))
FRAME = [
    (("exact", 0, True), P("table", N.TABLE_AUTO, 1, 0, "link")),
    (("exact", 0, False), P("table", N.TABLE_AUTO, 1, 0)),
    (("exact", 2, False), P("table", N.TABLE_AUTO, 1, 2)),
    (("exact", -5, True), P("table", N.TABLE_AUTO, 6, -5, "link")),
    (("parallel", 0, True), P("table", N.PARSE_PARALLEL, 1, 0)),
    (("parallel", -1, False), P("table", N.PARSE_PARALLEL, 2, -1)),
    (("hc", 3, True), P("hc", level=3, history="hist")),
    (("hc", 9, False), P("hc", level=9)),
    (("hc", 12, True), P("hc", level=12, history="hist")),
    (("optimal", 9, False), P("opt", level=9)),
    (("fast", 0, True), (ValueError, BAD_PARSE)),
    ((None, 0, True), (ValueError, BAD_PARSE)),
    ((3, 9, False), (ValueError, BAD_PARSE)),
    (("hc", 2, True), (ValueError, LOW.format("hc"))),
    (("hc", 0, False), (ValueError, LOW.format("hc"))),
    (("optimal", 2, False), (ValueError, LOW.format("optimal"))),
    (("optimal", 0, True), (ValueError, LOW.format("optimal"))),
    (("exact", 3, True), (NotImplementedError, HIGH)),
    (("exact", 9, False), (NotImplementedError, HIGH)),
    (("parallel", 3, False), (NotImplementedError, HIGH)),
    (("optimal", 9, True), (F.LinkedOptimalError, LINKED_OPT)),
    (("optimal", 3, True), (F.LinkedOptimalError, LINKED_OPT)),
]


def _check(call, want):
    if isinstance(want, N.Parse):
        got = call()
        assert type(got) is N.Parse and got == want
        return
    kind, message = want
    with pytest.raises(kind) as e:
        call()
    assert type(e.value) is kind and str(e.value) == message


@pytest.mark.parametrize("kw,want", BLOCK, ids=[str(i) for i in range(len(BLOCK))])
def test_block_arguments_resolve(kw, want):
    _check(lambda: B.resolve_parse(**kw), want)


@pytest.mark.parametrize("args,want", FRAME, ids=[str(i) for i in range(len(FRAME))])
def test_frame_arguments_resolve(args, want):
    _check(lambda: F.resolve_parse(*args), want)


def test_the_description_is_immutable_and_every_resolved_pair_has_a_launch():
    p = F.resolve_parse("hc", 9, True)
    with pytest.raises(AttributeError):
        p.level = 3
    for want in [w for _, w in BLOCK + FRAME if isinstance(w, N.Parse)]:
        assert (want.launcher, want.history) in N._BLOCK_LAUNCH


def test_linked_optimal_is_both_errors():
    assert issubclass(F.LinkedOptimalError, NotImplementedError) and issubclass(F.LinkedOptimalError, ValueError)

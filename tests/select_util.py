"""Shared inputs of the select tests (CPU and GPU): the boundary table of every source, op
and kind, the seeded mix, and the conversion of the restatement's clauses (tests/
select_ref.py) into the C ABI's structs over any memory (host numpy or device tensors)."""
import struct

import numpy as np

import select_ref as R
from iggy_amd import abi

FIELDS = ("ids", "checksums", "offsets", "timestamps", "origin_timestamps", "payload_lengths",
          "user_headers_lengths", "payload_starts", "user_headers_starts", "payloads", "user_headers")


def column(rows):
    """rows: (kind, length, stored bytes) per message -> a host column dict."""
    n = len(rows)
    col = {"value_kinds": np.zeros(n, np.uint8), "value_lengths": np.zeros(n, np.uint8),
           "values16": np.zeros((n, 16), np.uint8)}
    for i, (k, l, b) in enumerate(rows):
        col["value_kinds"][i], col["value_lengths"][i] = k, l
        b = bytes(b)[:16]
        col["values16"][i, :len(b)] = np.frombuffer(b, np.uint8)
    return col


def abi_spec(clauses, ptr, mask=None):
    """The restatement's clauses as an abi.SelectSpec; ptr(array) -> the address the entry
    point is to read that array at (host or device)."""
    out = []
    for c in clauses:
        col = None
        if c.column is not None:
            col = abi.HeaderColumn(*(ptr(c.column[k]) if c.column.get(k) is not None else None
                                     for k in ("value_kinds", "value_lengths")), None,
                                   ptr(c.column["values16"]) if c.column.get("values16") is not None else None)
        out.append(abi.SelectClause.make(c.source, c.op, c.operand, c.kind, col,
                                         ptr(c.status) if c.status is not None else None, c.length))
    return abi.SelectSpec.make(out, ptr(mask) if mask is not None else None)


def src_struct(src, cap, ptr, cap_p=None, cap_u=None):
    """The source dict as an abi.UnpackedMessages (missing arrays NULL, byte capacities the arrays' sizes)."""
    def size(k, c):
        return c if c is not None else src[k].size if src.get(k) is not None else 0
    return abi.UnpackedMessages(cap, size("payloads", cap_p), size("user_headers", cap_u),
                                *(ptr(src[k]) if src.get(k) is not None else None for k in FIELDS))


def make_source(pl, uh=None, seed=1):
    """A host source of len(pl) messages with the given payload / user-header lengths."""
    rng = np.random.default_rng(seed)
    pl = np.asarray(pl, dtype=np.uint32)
    n = pl.size
    uh = np.zeros(n, np.uint32) if uh is None else np.asarray(uh, dtype=np.uint32)
    return {
        "ids": rng.integers(0, 2**64, size=2 * n, dtype=np.uint64),
        "checksums": rng.integers(0, 2**64, size=n, dtype=np.uint64),
        "offsets": (np.uint64(1000) + np.arange(n, dtype=np.uint64)),
        "timestamps": np.full(n, 1_800_000_000_000_000, np.uint64) + (np.arange(n, dtype=np.uint64) // np.uint64(max(n // 2, 1))),
        "origin_timestamps": np.uint64(1_700_000_000_000_000) + rng.integers(0, 10**6, size=n).astype(np.uint64),
        "payload_lengths": pl, "user_headers_lengths": uh,
        "payload_starts": np.concatenate([[0], np.cumsum(pl, dtype=np.uint64)]).astype(np.uint64),
        "user_headers_starts": np.concatenate([[0], np.cumsum(uh, dtype=np.uint64)]).astype(np.uint64),
        "payloads": rng.integers(0, 256, size=int(pl.sum()), dtype=np.uint8),
        "user_headers": rng.integers(0, 256, size=int(uh.sum()), dtype=np.uint8),
    }


# ------------------------------------------------------------------ boundary table
def _i(v, size, signed):
    return int(v).to_bytes(size, "little", signed=signed)


def _f32(bits):
    return struct.pack("<I", bits)


def _f64(bits):
    return struct.pack("<Q", bits)


def header_groups():
    """kind group name -> [(kind, values as stored bytes, ops)]: every kind at its boundary values."""
    ints = {}
    for kind, size in ((R.K_INT8, 1), (R.K_INT16, 2), (R.K_INT32, 4), (R.K_INT64, 8), (R.K_INT128, 16)):
        b = 8 * size
        ints[kind] = [_i(v, size, True) for v in (-(1 << (b - 1)), -1, 0, 1, (1 << (b - 1)) - 1)]
    uints = {}
    for kind, size in ((R.K_UINT8, 1), (R.K_UINT16, 2), (R.K_UINT32, 4), (R.K_UINT64, 8), (R.K_UINT128, 16)):
        b = 8 * size
        uints[kind] = [_i(v, size, False) for v in (0, 1, (1 << (b - 1)) - 1, 1 << (b - 1), (1 << b) - 1)]
    f32 = [_f32(x) for x in (0xFF800000, 0xBFC00000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x007FFFFF,
                             0x3FC00000, 0x7F800000, 0x7FC00000, 0xFFC00001)]
    f64 = [_f64(x) for x in (0xFFF0000000000000, 0xBFF8000000000000, 0x8000000000000001, 0x8000000000000000, 0,
                             1, 0x000FFFFFFFFFFFFF, 0x3FF8000000000000, 0x7FF0000000000000, 0x7FF8000000000000,
                             0xFFF8000000000001)]
    eq = (R.OP_EQ, R.OP_NE)
    return {
        "signed": [(k, v, R.COMPARE_OPS) for k, v in ints.items()],
        "unsigned": [(k, v, R.COMPARE_OPS) for k, v in uints.items()],
        "float32": [(R.K_FLOAT32, f32, R.COMPARE_OPS)],
        "float64": [(R.K_FLOAT64, f64, R.COMPARE_OPS)],
        "bool": [(R.K_BOOL, [b"\x00", b"\x01"], eq)],
    }


S15, S16 = b"fifteen-bytes-1", b"sixteen-bytes-16"
assert (len(S15), len(S16)) == (15, 16)


def text_rows(kind):
    """Stored String / Raw rows: lengths 1, 15, 16, a longer value, and a stored length 17
    whose first 16 bytes match the 16-byte operand."""
    other = R.K_RAW if kind == R.K_STRING else R.K_STRING
    return [(kind, 1, b"a"), (kind, 1, b"b"), (kind, 15, S15), (kind, 16, S16), (kind, 20, b"a-longer-value-of-20"),
            (kind, 17, S16 + b"!"), (kind, 2, b"a\x00"), (0, 0, b""), (other, 1, b"a"), (other, 16, S16)]


TEXT_OPERANDS = (b"a", b"b", S15, S16, b"a\x00")


def header_cases():
    """-> [(group, column, [clause, ...])]: one column per kind (its boundary values, an absent
    row, a row of another kind with the same bytes), one clause per op and operand."""
    cases = []
    for group, kinds in header_groups().items():
        for kind, values, ops in kinds:
            size = len(values[0])
            other = next(k for k, s in R.KIND_SIZE.items() if s == size and k != kind)
            rows = [(kind, size, v) for v in values] + [(0, 0, b"")] + [(other, size, values[1])]
            col = column(rows)
            cl = [R.clause(R.SEL_HEADER, op, v, kind, col) for op in ops for v in values]
            cl += [R.clause(R.SEL_HEADER, op, column=col) for op in (R.OP_PRESENT, R.OP_ABSENT)]
            cases.append((group, col, cl))
    for kind in (R.K_STRING, R.K_RAW):
        col = column(text_rows(kind))
        cl = [R.clause(R.SEL_HEADER, op, v, kind, col) for op in (R.OP_EQ, R.OP_NE) for v in TEXT_OPERANDS]
        cases.append(("text", col, cl))
    return cases


def plain_cases():
    """-> (source dict of boundary values, [clause, ...]) for the u64 / u32 / u128 sources."""
    u64 = np.array([0, 1, 2**63 - 1, 2**63, 2**64 - 1, 5], dtype=np.uint64)
    u32 = np.array([0, 1, 2**31 - 1, 2**31, 2**32 - 1, 5], dtype=np.uint32)
    ids = np.array([0, 0, 2**64 - 1, 0, 0, 1, 2**64 - 1, 2**64 - 1, 0, 2**63, 5, 0], dtype=np.uint64)
    src = {"offsets": u64, "timestamps": u64[::-1].copy(), "origin_timestamps": np.roll(u64, 2),
           "payload_lengths": u32, "user_headers_lengths": u32[::-1].copy(), "ids": ids}
    cl = []
    for s in R.U64_SOURCES:
        cl += [R.clause(s, op, _i(int(v), 8, False)) for op in R.COMPARE_OPS for v in u64[:5]]
    for s in R.U32_SOURCES:
        cl += [R.clause(s, op, _i(int(v), 4, False)) for op in R.COMPARE_OPS for v in u32[:5]]
    for j in range(5):
        v = int(ids[2 * j]) | (int(ids[2 * j + 1]) << 64)
        cl += [R.clause(R.SEL_ID, op, _i(v, 16, False)) for op in R.COMPARE_OPS]
    return src, cl


# ------------------------------------------------------------------ refusals
def malformed_specs():
    """name -> (source dict, clauses) that both entry points refuse synchronously."""
    src = make_source([3, 4, 5])
    col = column([(R.K_INT32, 4, b"\x01\x00\x00\x00")] * 3)
    text = column([(R.K_STRING, 1, b"a")] * 3)
    status = np.zeros((3, 4), np.uint32)
    ok = R.clause(R.SEL_OFFSET, R.OP_GE, bytes(8))
    i32 = bytes(4)
    no = lambda d, k: {x: v for x, v in d.items() if x != k}  # noqa: E731
    bad = {
        "nine clauses": (src, [ok] * 9),
        "source 0": (src, [R.clause(0, R.OP_EQ, bytes(8))]),
        "source 9": (src, [R.clause(9, R.OP_EQ, bytes(8))]),
        "op 0": (src, [R.clause(R.SEL_OFFSET, 0, bytes(8))]),
        "op 9": (src, [R.clause(R.SEL_OFFSET, 9, bytes(8))]),
        "header op 0": (src, [R.clause(R.SEL_HEADER, 0, i32, R.K_INT32, col)]),
        "header op 9": (src, [R.clause(R.SEL_HEADER, 9, i32, R.K_INT32, col)]),
        "present on offsets": (src, [R.clause(R.SEL_OFFSET, R.OP_PRESENT, bytes(8))]),
        "absent on ids": (src, [R.clause(R.SEL_ID, R.OP_ABSENT, bytes(16))]),
        "no offsets array": (no(src, "offsets"), [ok]),
        "no timestamps array": (no(src, "timestamps"), [R.clause(R.SEL_TIMESTAMP, R.OP_EQ, bytes(8))]),
        "no origin array": (no(src, "origin_timestamps"), [R.clause(R.SEL_ORIGIN_TIMESTAMP, R.OP_EQ, bytes(8))]),
        "no payload_lengths array": (no(src, "payload_lengths"), [R.clause(R.SEL_PAYLOAD_LENGTH, R.OP_EQ, bytes(4))]),
        "no user_headers_lengths array": (no(src, "user_headers_lengths"),
                                          [R.clause(R.SEL_USER_HEADERS_LENGTH, R.OP_EQ, bytes(4))]),
        "no ids array": (no(src, "ids"), [R.clause(R.SEL_ID, R.OP_EQ, bytes(16))]),
        "no column": (src, [R.clause(R.SEL_HEADER, R.OP_PRESENT)]),
        "no value_kinds": (src, [R.clause(R.SEL_HEADER, R.OP_EQ, i32, R.K_INT32, no(col, "value_kinds"))]),
        "no values16": (src, [R.clause(R.SEL_HEADER, R.OP_EQ, i32, R.K_INT32, no(col, "values16"))]),
        "no value_lengths for a String": (src, [R.clause(R.SEL_HEADER, R.OP_EQ, b"a", R.K_STRING,
                                                         no(text, "value_lengths"))]),
        "no status": (src, [R.clause(R.SEL_HEADER_STATUS)]),
        "kind 0": (src, [R.clause(R.SEL_HEADER, R.OP_EQ, i32, 0, col)]),
        "kind 16": (src, [R.clause(R.SEL_HEADER, R.OP_EQ, i32, 16, col)]),
        "Int32 of 3 bytes": (src, [R.clause(R.SEL_HEADER, R.OP_EQ, bytes(3), R.K_INT32, col)]),
        "Uint128 of 8 bytes": (src, [R.clause(R.SEL_HEADER, R.OP_EQ, bytes(8), R.K_UINT128, col)]),
        "Float64 of 4 bytes": (src, [R.clause(R.SEL_HEADER, R.OP_EQ, bytes(4), R.K_FLOAT64, col)]),
        "String of 0 bytes": (src, [R.clause(R.SEL_HEADER, R.OP_EQ, b"", R.K_STRING, text)]),
        "Raw of 17 bytes": (src, [R.clause(R.SEL_HEADER, R.OP_EQ, bytes(16), R.K_RAW, text, length=17)]),
        "String <": (src, [R.clause(R.SEL_HEADER, R.OP_LT, b"a", R.K_STRING, text)]),
        "Raw >=": (src, [R.clause(R.SEL_HEADER, R.OP_GE, b"a", R.K_RAW, text)]),
        "Bool <=": (src, [R.clause(R.SEL_HEADER, R.OP_LE, b"\x01", R.K_BOOL, col)]),
        "a good clause before a bad one": (src, [ok, R.clause(R.SEL_HEADER, R.OP_GT, b"\x01", R.K_BOOL, col)]),
    }
    good = {
        "status without op": (src, [R.clause(R.SEL_HEADER_STATUS, status=status)]),
        "present without kind": (src, [R.clause(R.SEL_HEADER, R.OP_PRESENT, column=no(col, "values16"))]),
        "eight clauses": (src, [ok] * 8),
        "no clause": (src, []),
    }
    return bad, good


# ------------------------------------------------------------------ seeded mix
MIX_SEED = 4105


def seeded_mix(n=5000, seed=MIX_SEED):
    """-> (source, mask, [spec, ...]): n messages, three header columns and a status array,
    eight specs of 1..8 clauses that use every source and op."""
    rng = np.random.default_rng(seed)
    src = make_source(rng.integers(0, 200, size=n), rng.integers(0, 2, size=n) * rng.integers(1, 60, size=n), seed)
    src["offsets"] = np.uint64(2**63 - n // 2) + np.arange(n, dtype=np.uint64)  # crosses 2^63
    tenant = column([(R.K_INT32, 4, _i(int(v), 4, True)) if p else (0, 0, b"")
                     for v, p in zip(rng.integers(-500, 1500, size=n), rng.random(n) < 0.9)])
    route = column([((R.K_STRING, len(v), v) if p else (R.K_RAW, len(v), v) if q else (0, 0, b""))
                    for v, p, q in zip(rng.choice([b"eu", b"us", b"eu-west-1-zone-b-rack-17"], size=n),
                                       rng.random(n) < 0.8, rng.random(n) < 0.5)])
    score = column([(R.K_FLOAT64, 8, struct.pack("<d", v)) for v in
                    rng.choice([-1.5, -0.0, 0.0, 2.5, float("nan"), 5e-324, float("inf")], size=n)])
    status = np.zeros((n, 4), np.uint32)
    status[rng.random(n) < 0.05, 0] = 2
    mask = (rng.random(n) < 0.7).astype(np.uint8)

    def q(a, f):
        return int(np.sort(np.asarray(a))[int(f * (len(a) - 1))])

    u8 = lambda v: _i(v, 8, False)  # noqa: E731
    H = R.SEL_HEADER
    specs = [
        ([R.clause(R.SEL_OFFSET, R.OP_GE, u8(q(src["offsets"], 0.1))),
          R.clause(R.SEL_ORIGIN_TIMESTAMP, R.OP_LT, u8(q(src["origin_timestamps"], 0.95))),
          R.clause(R.SEL_PAYLOAD_LENGTH, R.OP_NE, _i(7, 4, False)),
          R.clause(R.SEL_USER_HEADERS_LENGTH, R.OP_LE, _i(50, 4, False)),
          R.clause(R.SEL_ID, R.OP_GT, _i(1 << 123, 16, False)),
          R.clause(H, R.OP_PRESENT, column=tenant),
          R.clause(R.SEL_HEADER_STATUS, status=status),
          R.clause(H, R.OP_LE, struct.pack("<d", 2.5), R.K_FLOAT64, score)], None),
        ([R.clause(H, R.OP_EQ, b"eu", R.K_STRING, route)], None),
        ([R.clause(H, R.OP_NE, b"eu", R.K_STRING, route),
          R.clause(R.SEL_TIMESTAMP, R.OP_EQ, u8(int(src["timestamps"][0])))], None),
        ([R.clause(H, R.OP_GE, _i(-100, 4, True), R.K_INT32, tenant),
          R.clause(H, R.OP_LT, _i(1200, 4, True), R.K_INT32, tenant)], None),
        ([R.clause(R.SEL_PAYLOAD_LENGTH, R.OP_GT, _i(30, 4, False)),
          R.clause(R.SEL_OFFSET, R.OP_LE, u8(q(src["offsets"], 0.9)))], mask),
        ([R.clause(H, R.OP_ABSENT, column=route), R.clause(R.SEL_TIMESTAMP, R.OP_NE, u8(int(src["timestamps"][0])))],
         None),
        ([R.clause(R.SEL_USER_HEADERS_LENGTH, R.OP_EQ, _i(0, 4, False)),
          R.clause(R.SEL_ID, R.OP_LE, _i(7 << 125, 16, False))], None),
        ([R.clause(H, R.OP_GT, struct.pack("<d", -1.0), R.K_FLOAT64, score),
          R.clause(R.SEL_ORIGIN_TIMESTAMP, R.OP_GE, u8(q(src["origin_timestamps"], 0.1))),
          R.clause(R.SEL_PAYLOAD_LENGTH, R.OP_LT, _i(180, 4, False)),
          R.clause(R.SEL_USER_HEADERS_LENGTH, R.OP_GE, _i(1, 4, False))], None),
        ([], mask),
    ]
    return src, specs

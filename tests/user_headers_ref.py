"""Plain-Python restatement of the reference's user-header decode, the expected values of
the user-header tests (never the code under test):

  validate_user_headers          core/binary_protocol/src/primitives/user_headers.rs:84-139
  headers_from_validated_slice   core/common/src/wire_conversions.rs:802-840 (UnknownKinds::Reject)
  HeaderKind::expected_size      core/common/src/types/message/user_headers.rs:272-281

decode(buf) -> (status, pairs, {(key_kind, key_bytes) -> (value_kind, pos, len, bytes)})
with status = (kind, reason, offset, detail) as iggy_header_status carries it. Pinned on
the CPU by tests/golden/user_headers_vectors.json (tests/test_user_headers_cpu.py)."""
import struct

OK = 0
ERR_UNEXPECTED_EOF = 1
ERR_VALIDATION = 2
ERR_INVALID_HEADER_KEY = 27
ERR_INVALID_HEADER_VALUE = 28
ERR_INVALID_HEADER_KIND = 29
V_HEADER_KIND_ZERO = 11
V_HEADER_FIELD_LENGTH = 12
V_HEADER_ODD_ENTRIES = 13
MAX_FIELD_LENGTH = 255

# kind code -> fixed size (None: Raw / String, any length in 1..=255)
EXPECTED_SIZE = {1: None, 2: None, 3: 1, 4: 1, 5: 2, 6: 4, 7: 8, 8: 16, 9: 1, 10: 2, 11: 4, 12: 8, 13: 16,
                 14: 4, 15: 8}
STATUS_OK = (OK, 0, 0, 0)


def tlv(kind: int, data: bytes, length=None) -> bytes:
    return bytes([kind]) + struct.pack("<I", len(data) if length is None else length) + bytes(data)


def pair(key_kind: int, key: bytes, value_kind: int, value: bytes) -> bytes:
    return tlv(key_kind, key) + tlv(value_kind, value)


def validate(buf: bytes):
    """validate_user_headers -> (status, [(kind, data_pos, length)] in walk order or None)."""
    n = len(buf)
    pos = 0
    tlvs = []
    while pos < n:
        kind = buf[pos]
        if kind == 0:
            return (ERR_VALIDATION, V_HEADER_KIND_ZERO, pos, 0), None
        pos += 1
        if pos + 4 > n:
            return (ERR_UNEXPECTED_EOF, 0, pos, 4), None
        (length,) = struct.unpack_from("<I", buf, pos)
        pos += 4
        if length == 0 or length > MAX_FIELD_LENGTH:
            return (ERR_VALIDATION, V_HEADER_FIELD_LENGTH, pos - 4, length), None
        if pos + length > n:
            return (ERR_UNEXPECTED_EOF, 0, pos, length), None
        tlvs.append((kind, pos, length))
        pos += length
    if len(tlvs) % 2:
        return (ERR_VALIDATION, V_HEADER_ODD_ENTRIES, 0, len(tlvs)), None
    return STATUS_OK, tlvs


def decode(buf: bytes):
    buf = bytes(buf)
    status, tlvs = validate(buf)
    if status != STATUS_OK:
        return status, 0, {}
    headers = {}
    for j in range(0, len(tlvs), 2):
        (kk, kp, kl), (vk, vp, vl) = tlvs[j], tlvs[j + 1]
        start = kp - 5  # the pair's key-kind byte
        if kk not in EXPECTED_SIZE:
            return (ERR_INVALID_HEADER_KIND, kk, start, 0), 0, {}
        if vk not in EXPECTED_SIZE:
            return (ERR_INVALID_HEADER_KIND, vk, start, 0), 0, {}
        if EXPECTED_SIZE[kk] is not None and EXPECTED_SIZE[kk] != kl:
            return (ERR_INVALID_HEADER_KEY, 0, start, 0), 0, {}
        if EXPECTED_SIZE[vk] is not None and EXPECTED_SIZE[vk] != vl:
            return (ERR_INVALID_HEADER_VALUE, 0, start, 0), 0, {}
        headers[(kk, buf[kp:kp + kl])] = (vk, vp, vl, buf[vp:vp + vl])  # BTreeMap::insert: the last wins
    return STATUS_OK, len(tlvs) // 2, headers


def lookup(decoded, key):
    """(value_kind, pos, len, values16) of key = (kind, bytes) as the columns hold it."""
    status, _, headers = decoded
    hit = headers.get((key[0], bytes(key[1]))) if status == STATUS_OK else None
    if hit is None:
        return 0, 0, 0, bytes(16)
    vk, vp, vl, vb = hit
    return vk, vp, vl, (vb[:16] + bytes(16))[:16]

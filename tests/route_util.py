"""Shared inputs of the route tests (CPU and GPU): the conversion of the restatement's spec
(tests/route_ref.py) into the C ABI's struct over any memory (host numpy or device
tensors), header blobs with one key per message, and the malformed specs."""
import json
import os

import numpy as np

import route_ref as R
import select_util as U
from iggy_amd import abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xxh32_vectors.json")


def vectors():
    with open(GOLDEN) as f:
        return [(bytes.fromhex(v["data"]), v["seed"], v["hash"]) for v in json.load(f)["vectors"]]


def abi_spec(spec, ptr):
    """The restatement's Spec as an abi.RouteSpec; ptr(array) -> the address the entry point
    is to read that array at (host or device)."""
    col = None
    if spec.column is not None:
        col = abi.HeaderColumn(*(ptr(spec.column[k]) if spec.column.get(k) is not None else None
                                 for k in ("value_kinds", "value_lengths", "value_pos")), None)
    return abi.RouteSpec.make(spec.partitions, spec.key_source, spec.absent,
                              ptr(spec.keys) if spec.keys is not None else None, spec.key_length, spec.key_stride,
                              ptr(spec.partition_ids) if spec.partition_ids is not None else None, col,
                              ptr(spec.mask) if spec.mask is not None else None)


def header_source(keys, pl=None, seed=1):
    """A host source whose message i has the header bytes [i % 5 filler bytes | keys[i]] (no
    header bytes for keys[i] None) and the column that points at the key -> (src, column)."""
    n = len(keys)
    blobs = [b"" if k is None else bytes([0x40 + i % 7] * (i % 5)) + k for i, k in enumerate(keys)]
    src = U.make_source(np.arange(n) % 13 if pl is None else pl, [len(b) for b in blobs], seed)
    src["user_headers"] = np.frombuffer(b"".join(blobs) or b"", dtype=np.uint8).copy()
    col = {"value_kinds": np.array([0 if k is None else 2 for k in keys], np.uint8),
           "value_lengths": np.array([0 if k is None else len(k) for k in keys], np.uint8),
           "value_pos": np.array([0 if k is None else i % 5 for i, k in enumerate(keys)], np.uint32)}
    return src, col


def malformed_specs():
    """-> (bad, good): name -> (source dict, Spec) that both entry points refuse / accept."""
    src, col = header_source([b"a", None, b"bcd"])
    keys = np.zeros((3, 8), np.uint8)
    ids = np.zeros(3, np.uint32)
    no = lambda d, k: {x: v for x, v in d.items() if x != k}  # noqa: E731
    S = R.Spec
    bad = {
        "0 partitions": (src, S(0, R.KEY_ID)),
        "257 partitions": (src, S(257, R.KEY_ID)),
        "key source 0": (src, S(3, 0)),
        "key source 5": (src, S(3, 5)),
        "absent == partitions": (src, S(3, R.KEY_HEADER, 3, column=col)),
        "absent above partitions, by id": (src, S(3, R.KEY_ID, 7)),
        "bytes without keys": (src, S(3, R.KEY_BYTES, key_length=4, key_stride=8)),
        "bytes of length 0": (src, S(3, R.KEY_BYTES, key_length=0, key_stride=8, keys=keys)),
        "bytes of length 256": (src, S(3, R.KEY_BYTES, key_length=256, key_stride=256, keys=keys)),
        "stride below the length": (src, S(3, R.KEY_BYTES, key_length=8, key_stride=7, keys=keys)),
        "partition without ids": (src, S(3, R.KEY_PARTITION)),
        "header without value_kinds": (src, S(3, R.KEY_HEADER, column=no(col, "value_kinds"))),
        "header without value_lengths": (src, S(3, R.KEY_HEADER, column=no(col, "value_lengths"))),
        "header without value_pos": (src, S(3, R.KEY_HEADER, column=no(col, "value_pos"))),
        "header without a column": (src, S(3, R.KEY_HEADER)),
        "header without user_headers_starts": (no(src, "user_headers_starts"), S(3, R.KEY_HEADER, column=col)),
        "header without user_headers": (no(src, "user_headers"), S(3, R.KEY_HEADER, column=col)),
        "id without ids": (no(src, "ids"), S(3, R.KEY_ID)),
    }
    good = {
        "by id": (src, S(3, R.KEY_ID)),
        "one partition": (src, S(1, R.KEY_ID)),
        "256 partitions": (src, S(256, R.KEY_ID)),
        "header, absent dropped": (src, S(3, R.KEY_HEADER, column=col)),
        "header, absent to the last": (src, S(3, R.KEY_HEADER, 2, column=col)),
        "bytes, stride == length": (src, S(3, R.KEY_BYTES, key_length=8, key_stride=8, keys=keys)),
        "bytes of 1": (src, S(3, R.KEY_BYTES, key_length=1, key_stride=8, keys=keys)),
        "partition ids": (src, S(3, R.KEY_PARTITION, partition_ids=ids)),
    }
    return bad, good

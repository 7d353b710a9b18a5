#!/usr/bin/env python3
"""Timing of the device user-header validation and key columns
(iggy_codec_user_headers_device / _arrays_device) alone: 1,048,576 messages x 1 KiB payload,
each with 4 header pairs (about 64 B of headers), 2 request keys.

The record is encoded on the device by the codec, decoded once (Verify) and unpacked once;
then each form is timed with HIP events, warm, median of --runs runs, next to a plain
device-to-device copy of exactly the bytes the kernel must read, in the same process (the
yardstick): the whole record for the record form (the headers lie between the payloads),
the header blob for the arrays form. Figures per form: ms, the ratio to the copy, and
algorithmic bytes (header bytes read + columns written) / time / 8 TB/s.

    python scripts/user_headers_timing.py [--runs 25] [--out profiles/user_headers_timing.json]

Prints one JSON line. Not part of bench.py; needs an MI355X."""
import argparse
import ctypes
import json
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
N_MSG = 1 << 20
PAYLOAD = 1024


def events_ms(torch, fn, runs, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def tlv(kind, data):
    return bytes([kind]) + struct.pack("<I", len(data)) + data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from iggy_amd import abi
    from iggy_amd.codec import Codec
    from iggy_amd.torch_io import to_device, to_host
    if not torch.cuda.is_available():
        sys.exit("user_headers_timing.py measures on an MI355X; no GPU found")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    cx = Codec(0)
    n = N_MSG
    # 4 pairs, 64 B: String route -> String, String seq -> Int64 (= the message index),
    # String tenant -> Uint32, Raw k -> Bool
    one = (tlv(2, b"route") + tlv(2, b"eu-1") + tlv(2, b"seq") + tlv(7, bytes(8)) +
           tlv(2, b"tenant") + tlv(11, bytes(4)) + tlv(1, b"k") + tlv(3, b"\x01"))
    uhl = len(one)
    seq_at = one.index(tlv(7, bytes(8))) + 5
    hdr = np.tile(np.frombuffer(one, dtype=np.uint8), (n, 1))
    hdr[:, seq_at:seq_at + 8] = np.arange(n, dtype=np.int64).view(np.uint8).reshape(n, 8)
    keys = [(abi.KIND_STRING, b"seq"), (abi.KIND_STRING, b"tenant")]
    with torch.cuda.stream(torch.cuda.Stream()):
        s = torch.cuda.current_stream().cuda_stream
        assert s != 0
        g = torch.Generator(device=dev)
        g.manual_seed(0x16619E3779B97F4A)
        pls = torch.full((n,), PAYLOAD, dtype=torch.int32, device=dev)
        uhls = torch.full((n,), uhl, dtype=torch.int32, device=dev)
        payload = torch.randint(0, 256, (n * PAYLOAD,), dtype=torch.uint8, device=dev, generator=g)
        d_hdr = to_device(hdr.reshape(-1), dev)
        ids = torch.randint(1, 2**62, (2 * n,), dtype=torch.int64, device=dev, generator=g)
        ots = 1_700_000_000_000_000 + torch.arange(n, dtype=torch.int64, device=dev)
        L = 256 + (48 + PAYLOAD + uhl) * n
        rec = torch.empty(L, dtype=torch.uint8, device=dev)
        eres = torch.zeros(ctypes.sizeof(abi.EncodeResult), dtype=torch.uint8, device=dev)
        raw = abi.RawMessages(n, ids.data_ptr(), ots.data_ptr(), payload.data_ptr(), pls.data_ptr(),
                              d_hdr.data_ptr(), uhls.data_ptr())
        torch.cuda.synchronize()
        assert cx.encode_device(raw, 1, rec.data_ptr(), L, eres.data_ptr(), s) == 0
        pos = torch.empty(n, dtype=torch.int64, device=dev)
        dres = torch.zeros(ctypes.sizeof(abi.DecodeResult), dtype=torch.uint8, device=dev)
        assert cx.decode_device(rec.data_ptr(), L, abi.INTEGRITY_VERIFY, pos.data_ptr(), n, dres.data_ptr(), s) == 0
        # the arrays form's input: the unpack's user_headers / starts
        blob = torch.empty(n * uhl, dtype=torch.uint8, device=dev)
        starts = torch.empty(n + 1, dtype=torch.int64, device=dev)
        um = abi.UnpackedMessages(n, 0, n * uhl)
        um.user_headers, um.user_headers_starts = blob.data_ptr(), starts.data_ptr()
        cursor = torch.zeros(4, dtype=torch.int64, device=dev)
        ures = torch.zeros(ctypes.sizeof(abi.UnpackResult), dtype=torch.uint8, device=dev)
        assert cx.unpack_device(rec.data_ptr(), L, pos.data_ptr(), dres.data_ptr(), um, cursor.data_ptr(),
                                ures.data_ptr(), s) == 0
        torch.cuda.synchronize()
        dr = abi.DecodeResult.from_buffer_copy(to_host(dres).tobytes())
        assert dr.error.kind == 0 and dr.frame_count == n, dr.error
        assert torch.equal(blob, d_hdr)

        status = torch.empty((n, 4), dtype=torch.int32, device=dev)
        pairs = torch.empty(n, dtype=torch.int32, device=dev)
        cols = [{"value_kinds": torch.empty(n, dtype=torch.uint8, device=dev),
                 "value_lengths": torch.empty(n, dtype=torch.uint8, device=dev),
                 "value_pos": torch.empty(n, dtype=torch.int32, device=dev),
                 "values16": torch.empty((n, 16), dtype=torch.uint8, device=dev)} for _ in keys]
        q = abi.HeaderColumns()
        q.cap_messages, q.nkeys = n, len(keys)
        q.status, q.pairs = status.data_ptr(), pairs.data_ptr()
        for k, (kind, key) in enumerate(keys):
            q.keys[k] = abi.HeaderKey.make(kind, key)
            q.columns[k] = abi.HeaderColumn(*(cols[k][f].data_ptr() for f in ("value_kinds", "value_lengths",
                                                                               "value_pos", "values16")))
        hres = torch.zeros(ctypes.sizeof(abi.HeaderColumnsResult), dtype=torch.uint8, device=dev)

        def record_form():
            assert cx.user_headers_device(rec.data_ptr(), L, pos.data_ptr(), dres.data_ptr(), q, hres.data_ptr(), s) == 0

        def arrays_form():
            assert cx.user_headers_arrays_device(blob.data_ptr(), starts.data_ptr(), cursor.data_ptr(), n, q,
                                                 hres.data_ptr(), s) == 0

        written = n * (16 + 4 + len(keys) * (1 + 1 + 4 + 16))
        res = {"script": "scripts/user_headers_timing.py", "device": torch.cuda.get_device_name(0), "messages": n,
               "payload_bytes": PAYLOAD, "header_bytes_per_message": uhl, "pairs_per_message": 4,
               "request_keys": len(keys), "runs": a.runs, "batch_bytes": L}
        for name, fn, src in (("record_form", record_form, rec), ("arrays_form", arrays_form, blob)):
            med, lo_ms, hi_ms = events_ms(torch, fn, a.runs)
            r = abi.HeaderColumnsResult.from_buffer_copy(to_host(hres).tobytes())
            assert r.error.kind == 0 and (r.count, r.with_headers, r.invalid_messages) == (n, n, 0), r.error
            assert r.found[0] == n and r.found[1] == n
            seq = cols[0]["values16"].view(torch.int64)[:, 0]
            assert torch.equal(seq, torch.arange(n, dtype=torch.int64, device=dev))
            assert int(pairs.min()) == 4 and int(cols[1]["value_kinds"].max()) == abi.KIND_UINT32
            dst = torch.empty_like(src)
            cmed, clo, chi = events_ms(torch, lambda: dst.copy_(src), a.runs)
            alg = n * uhl + written + (8 * n if name == "record_form" else 8 * (n + 1))
            res[name] = {"ms": round(med, 4), "min_ms": round(lo_ms, 4), "max_ms": round(hi_ms, 4),
                         "d2d_copy_bytes": int(src.numel()), "d2d_copy_ms": round(cmed, 4),
                         "d2d_copy_hbm_frac": round(2 * src.numel() / (cmed * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                         "ratio_to_copy": round(med / cmed, 3), "algorithmic_bytes": alg,
                         "hbm_frac": round(alg / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    cx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

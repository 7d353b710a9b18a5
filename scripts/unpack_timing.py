#!/usr/bin/env python3
"""Timing of the consumer unpack (iggy_codec_unpack_batch_device) alone, on the C2 record
(1,048,576 x 1 KiB) and the C3 record (1,048,576 messages, payloads U[64, 4096]).

Each record is encoded on the device by the codec and decoded once (Verify); then the
unpack is timed with HIP events, warm, median of --runs runs, next to a plain device-to-
device copy of batch_length bytes in the same process (the yardstick). Three figures per
record: ms, algorithmic bytes / time / 8 TB/s (the record read once plus every array
written), and the ratio to the plain copy. Two partial unpacks give the phase split:
"index" = fields + scan + starts (no byte copy), "bytes" = lengths + scan + starts + copy
(no fixed-width fields). The unpacked payloads are compared with the encoder's input.

    python scripts/unpack_timing.py [--runs 25] [--out profiles/unpack_timing.json]

Prints one JSON line. Not part of bench.py; needs an MI355X."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
N_MSG = 1 << 20


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


def one(cx, name, lo, hi, runs):
    import torch
    from iggy_amd import abi
    from iggy_amd.torch_io import to_host

    dev = torch.device("cuda:0")
    n = N_MSG
    g = torch.Generator(device=dev)
    g.manual_seed(0x16619E3779B97F4A)
    pls = (torch.full((n,), lo, dtype=torch.int32, device=dev) if lo == hi
           else torch.randint(lo, hi + 1, (n,), dtype=torch.int32, device=dev, generator=g))
    total_pl = int(pls.sum().item())
    payload = torch.randint(0, 256, (total_pl,), dtype=torch.uint8, device=dev, generator=g)
    ids = torch.randint(1, 2**62, (2 * n,), dtype=torch.int64, device=dev, generator=g)
    ots = 1_700_000_000_000_000 + torch.arange(n, dtype=torch.int64, device=dev)
    L = 256 + 48 * n + total_pl
    rec = torch.empty(L, dtype=torch.uint8, device=dev)
    eres = torch.zeros(ctypes.sizeof(abi.EncodeResult), dtype=torch.uint8, device=dev)
    raw = abi.RawMessages(n, ids.data_ptr(), ots.data_ptr(), payload.data_ptr(), pls.data_ptr(), None, None)
    s = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    assert cx.encode_device(raw, 1, rec.data_ptr(), L, eres.data_ptr(), s) == 0
    pos = torch.empty(n, dtype=torch.int64, device=dev)
    dres = torch.zeros(ctypes.sizeof(abi.DecodeResult), dtype=torch.uint8, device=dev)
    assert cx.decode_device(rec.data_ptr(), L, abi.INTEGRITY_VERIFY, pos.data_ptr(), n, dres.data_ptr(), s) == 0
    torch.cuda.synchronize()
    dr = abi.DecodeResult.from_buffer_copy(to_host(dres).tobytes())
    assert dr.error.kind == 0 and dr.frame_count == n, dr.error

    i64 = torch.int64
    o = {"ids": torch.empty(2 * n, dtype=i64, device=dev), "checksums": torch.empty(n, dtype=i64, device=dev),
         "offsets": torch.empty(n, dtype=i64, device=dev), "timestamps": torch.empty(n, dtype=i64, device=dev),
         "origin_timestamps": torch.empty(n, dtype=i64, device=dev),
         "payload_lengths": torch.empty(n, dtype=torch.int32, device=dev),
         "user_headers_lengths": torch.empty(n, dtype=torch.int32, device=dev),
         "payload_starts": torch.empty(n + 1, dtype=i64, device=dev),
         "user_headers_starts": torch.empty(n + 1, dtype=i64, device=dev),
         "payloads": torch.empty(total_pl, dtype=torch.uint8, device=dev),
         "user_headers": torch.empty(16, dtype=torch.uint8, device=dev)}
    order = ("ids", "checksums", "offsets", "timestamps", "origin_timestamps", "payload_lengths",
             "user_headers_lengths", "payload_starts", "user_headers_starts", "payloads", "user_headers")

    def struct(keys):
        return abi.UnpackedMessages(n, total_pl, 16, *(o[k].data_ptr() if k in keys else None for k in order))

    ures = torch.zeros(ctypes.sizeof(abi.UnpackResult), dtype=torch.uint8, device=dev)
    variants = {
        "full": struct(order),
        "index": struct([k for k in order if k not in ("payloads", "user_headers")]),
        "bytes": struct(("payload_starts", "user_headers_starts", "payloads", "user_headers")),
    }

    def run(u):
        rc = cx.unpack_device(rec.data_ptr(), L, pos.data_ptr(), dres.data_ptr(), u, None, ures.data_ptr(), s)
        assert rc == 0, rc

    out = {"workload": name, "batch_bytes": L, "messages": n, "runs": runs}
    fixed = n * (16 + 8 + 8 + 8 + 8 + 4 + 4) + 2 * 8 * (n + 1)
    # (the index pass reads the 48-B frame headers and the 8-B positions, not the payloads)
    alg = {"full": L + fixed + total_pl, "index": 56 * n + fixed, "bytes": L + 2 * 8 * (n + 1) + total_pl}
    for k, u in variants.items():
        med, lo_ms, hi_ms = events_ms(torch, lambda: run(u), runs)
        ur = abi.UnpackResult.from_buffer_copy(to_host(ures).tobytes())
        assert ur.error.kind == 0 and ur.count == n and ur.payload_bytes == total_pl, ur.error
        out[k] = {"ms": round(med, 4), "min_ms": round(lo_ms, 4), "max_ms": round(hi_ms, 4),
                  "algorithmic_bytes": alg[k], "hbm_frac": round(alg[k] / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    # the unpacked arrays are the encoder's input
    assert torch.equal(o["payloads"], payload) and torch.equal(o["payload_lengths"], pls)
    assert torch.equal(o["ids"], ids) and torch.equal(o["origin_timestamps"], ots)
    dst = torch.empty_like(rec)
    med, lo_ms, hi_ms = events_ms(torch, lambda: dst.copy_(rec), runs)
    out["d2d_copy"] = {"ms": round(med, 4), "min_ms": round(lo_ms, 4), "max_ms": round(hi_ms, 4),
                       "hbm_frac": round(2 * L / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    out["ratio_to_copy"] = round(out["full"]["ms"] / med, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from iggy_amd.codec import Codec
    if not torch.cuda.is_available():
        sys.exit("unpack_timing.py measures on an MI355X; no GPU found")
    torch.cuda.set_device(0)
    cx = Codec(0)
    # one explicit stream for the codec's work, the copies and the events (torch's default
    # stream is handle 0, which the C ABI reads as "the context's own stream")
    with torch.cuda.stream(torch.cuda.Stream()):
        assert torch.cuda.current_stream().cuda_stream != 0
        res = {"script": "scripts/unpack_timing.py", "device": torch.cuda.get_device_name(0),
               "c2": one(cx, "C2 record: 1,048,576 x 1 KiB", 1024, 1024, a.runs),
               "c3": one(cx, "C3 record: 1,048,576 msgs, payloads U[64,4096] B", 64, 4096, a.runs)}
    cx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timing of the device route (iggy_codec_route_messages_device) alone, on C2-shaped arrays
(1,048,576 x 1 KiB) built on the device.

The route is timed (HIP events, warm, median of --runs runs, one process) keyed by id into
1, 8 and 256 partitions, and once keyed by a 12-B header value (24 B of header bytes per
message) into 8. Per case the hash-only form (out = NULL: keys, scan, partition_of) is timed
too, which separates the index passes from the scatter, the starts and the byte copies. The
yardsticks, in the same process, are a plain device-to-device copy of the routed payload
bytes and select_messages at keep = 100 % over the same arrays (both share the copy form).
Every GPU step is checked: return codes, the device results, the partition of every message
against the host twin's XXH32 for a sample, the order against a stable torch sort, and the
routed payloads against a row gather.

    python scripts/route_timing.py [--runs 25] [--out profiles/route_timing.json] [--limit 600]

The GPU work runs in a child process under a time limit. Prints one JSON line. Not part of
bench.py; needs an MI355X."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_MSG = 1 << 20
L = 1024
ORDER = ("ids", "checksums", "offsets", "timestamps", "origin_timestamps", "payload_lengths",
         "user_headers_lengths", "payload_starts", "user_headers_starts", "payloads", "user_headers")


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


def measure(cx, runs):
    import numpy as np
    import torch

    from iggy_amd import abi
    from iggy_amd.codec import xxh32
    from iggy_amd.torch_io import to_host

    dev = torch.device("cuda:0")
    n, i64 = N_MSG, torch.int64
    g = torch.Generator(device=dev)
    g.manual_seed(0x16619E3779B97F4A)
    hb = 24  # header bytes per message; the key is bytes [5, 17)
    a = {"ids": torch.randint(1, 2**62, (2 * n,), dtype=i64, device=dev, generator=g),
         "checksums": torch.randint(1, 2**62, (n,), dtype=i64, device=dev, generator=g),
         "offsets": torch.arange(n, dtype=i64, device=dev), "timestamps": torch.full((n,), 17, dtype=i64, device=dev),
         "origin_timestamps": 1_700_000_000_000_000 + torch.arange(n, dtype=i64, device=dev),
         "payload_lengths": torch.full((n,), L, dtype=torch.int32, device=dev),
         "user_headers_lengths": torch.full((n,), hb, dtype=torch.int32, device=dev),
         "payload_starts": torch.arange(n + 1, dtype=i64, device=dev) * L,
         "user_headers_starts": torch.arange(n + 1, dtype=i64, device=dev) * hb,
         "payloads": torch.randint(0, 256, (n * L,), dtype=torch.uint8, device=dev, generator=g),
         "user_headers": torch.randint(0, 256, (n * hb,), dtype=torch.uint8, device=dev, generator=g)}
    src = abi.UnpackedMessages(n, n * L, n * hb, *(a[k].data_ptr() for k in ORDER))
    o = {k: torch.empty_like(v) for k, v in a.items()}
    out = abi.UnpackedMessages(n, n * L, n * hb, *(o[k].data_ptr() for k in ORDER))
    d_idx = torch.empty(n, dtype=i64, device=dev)
    d_of = torch.empty(n, dtype=torch.int32, device=dev)
    d_tab = torch.zeros((3, 257), dtype=i64, device=dev)
    d_cnt = torch.full((1,), n, dtype=i64, device=dev)
    d_res = torch.zeros(ctypes.sizeof(abi.RouteResult), dtype=torch.uint8, device=dev)
    d_sel = torch.zeros(ctypes.sizeof(abi.SelectResult), dtype=torch.uint8, device=dev)
    kinds = torch.full((n,), abi.KIND_STRING, dtype=torch.uint8, device=dev)
    lens = torch.full((n,), 12, dtype=torch.uint8, device=dev)
    pos = torch.full((n,), 5, dtype=torch.int32, device=dev)
    col = abi.HeaderColumn(kinds.data_ptr(), lens.data_ptr(), pos.data_ptr(), None)
    s = torch.cuda.current_stream().cuda_stream
    res = {"messages": n, "payload_bytes": n * L, "user_headers_bytes": n * hb, "runs": runs}

    sel_spec = abi.SelectSpec.make([], None)

    def select_all():
        assert cx.select_messages_device(src, d_cnt.data_ptr(), sel_spec, out, d_idx.data_ptr(), None,
                                         d_sel.data_ptr(), s) == 0

    smed, _, _ = events_ms(torch, select_all, runs)
    sr = abi.SelectResult.from_buffer_copy(to_host(d_sel).tobytes())
    assert sr.error.kind == 0 and sr.count == n and torch.equal(o["payloads"], a["payloads"]), sr.error
    dst = torch.empty(n * L, dtype=torch.uint8, device=dev)
    cmed, _, _ = events_ms(torch, lambda: dst.copy_(a["payloads"]), runs)
    del dst
    res["select_keep_100_ms"], res["d2d_copy_of_payloads_ms"] = round(smed, 4), round(cmed, 4)

    ids_h = to_host(a["ids"]).reshape(n, 2)
    uh_h = to_host(a["user_headers"]).reshape(n, hb)
    cases = [("id_1", 1, None), ("id_8", 8, None), ("id_256", 256, None), ("header_8", 8, col)]
    for name, parts, column in cases:
        spec = (abi.RouteSpec.make(parts, abi.ROUTE_KEY_ID) if column is None
                else abi.RouteSpec.make(parts, abi.ROUTE_KEY_HEADER, column=column))

        def run(full=True):
            rc = cx.route_messages_device(src, d_cnt.data_ptr(), spec, out if full else None, d_tab[0].data_ptr(),
                                          d_tab[1].data_ptr() if full else None, d_tab[2].data_ptr() if full else None,
                                          d_of.data_ptr(), d_idx.data_ptr() if full else None, d_res.data_ptr(), s)
            assert rc == 0, rc

        hmed, _, _ = events_ms(torch, lambda: run(False), runs)
        med, lo_ms, hi_ms = events_ms(torch, run, runs)
        r = abi.RouteResult.from_buffer_copy(to_host(d_res).tobytes())
        assert r.error.kind == 0 and (r.examined, r.count, r.dropped, r.payload_bytes) == (n, n, 0, n * L), r.error
        part = d_of.to(i64)
        for i in list(range(0, n, n // 64)) + [n - 1]:  # a sample against the host XXH32
            key = ids_h[i].tobytes() if column is None else uh_h[i, 5:17].tobytes()
            assert int(part[i].item()) == xxh32(key) % parts, (name, i)
        order = torch.sort(part, stable=True).indices
        assert torch.equal(d_idx, order) and torch.equal(o["offsets"], a["offsets"][order])
        assert torch.equal(o["payloads"].view(n, L), a["payloads"].view(n, L)[order])
        assert torch.equal(o["user_headers"].view(n, hb), a["user_headers"].view(n, hb)[order])
        first = torch.zeros(parts + 1, dtype=i64, device=dev)
        first[1:] = torch.cumsum(torch.bincount(part, minlength=parts), 0)
        assert torch.equal(d_tab[0, :parts + 1], first) and torch.equal(d_tab[1, :parts + 1], first * L)
        res[name] = {"partitions": parts, "ms": round(med, 4), "min_ms": round(lo_ms, 4), "max_ms": round(hi_ms, 4),
                     "hash_only_ms": round(hmed, 4), "ratio_to_select_keep_100": round(med / smed, 3),
                     "ratio_to_copy": round(med / cmed, 3)}
    return res


def child(runs):
    import torch

    from iggy_amd.codec import Codec
    if not torch.cuda.is_available():
        sys.exit("route_timing.py measures on an MI355X; no GPU found")
    torch.cuda.set_device(0)
    cx = Codec(0)
    # one explicit stream for the codec's work, the copies and the events (torch's default
    # stream is handle 0, which the C ABI reads as "the context's own stream")
    with torch.cuda.stream(torch.cuda.Stream()):
        assert torch.cuda.current_stream().cuda_stream != 0
        res = {"script": "scripts/route_timing.py", "device": torch.cuda.get_device_name(0),
               "c2": measure(cx, runs)}
    cx.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=600, help="seconds the GPU step may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.runs)
    # the GPU step in a fresh child process under a time limit; nothing is retried
    p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child",
                        "--runs", str(a.runs)], capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        sys.exit(p.returncode)
    line = p.stdout.strip().splitlines()[-1]
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timing of the device select (iggy_codec_select_messages_device) alone, on C2-shaped
arrays (1,048,576 x 1 KiB) and C3-shaped arrays (1,048,576 messages, payloads U[64, 4096]).

The source arrays are built on the device. Per shape the select is timed (HIP events, warm,
median of --runs runs, one process) at keep = 100 % (no mask, no clause), 50 % (a mask of
alternating messages), 1 % (a mask of every 100th) and with one Int32 header clause
(tenant < 50 of i % 100, no mask). The yardstick is a plain device-to-device copy of the
KEPT payload bytes in the same process; at keep = 100 % a second one is the unpack's
byte-copy form (lengths + scan + starts + the two copy launches, no fixed-width fields) of
a record that the codec encoded from the same arrays. Every GPU step is checked: return
codes, the device results, and the kept payloads against a torch gather.

    python scripts/select_timing.py [--runs 25] [--out profiles/select_timing.json]

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


def one(cx, name, lo, hi, runs):
    import torch
    from iggy_amd import abi
    from iggy_amd.torch_io import to_host

    dev = torch.device("cuda:0")
    n, i64 = N_MSG, torch.int64
    g = torch.Generator(device=dev)
    g.manual_seed(0x16619E3779B97F4A)
    pls = (torch.full((n,), lo, dtype=torch.int32, device=dev) if lo == hi
           else torch.randint(lo, hi + 1, (n,), dtype=torch.int32, device=dev, generator=g))
    starts = torch.zeros(n + 1, dtype=i64, device=dev)
    starts[1:] = torch.cumsum(pls.to(i64), 0)
    total = int(starts[-1].item())
    a = {"ids": torch.randint(1, 2**62, (2 * n,), dtype=i64, device=dev, generator=g),
         "checksums": torch.randint(1, 2**62, (n,), dtype=i64, device=dev, generator=g),
         "offsets": torch.arange(n, dtype=i64, device=dev), "timestamps": torch.full((n,), 17, dtype=i64, device=dev),
         "origin_timestamps": 1_700_000_000_000_000 + torch.arange(n, dtype=i64, device=dev),
         "payload_lengths": pls, "user_headers_lengths": torch.zeros(n, dtype=torch.int32, device=dev),
         "payload_starts": starts, "user_headers_starts": torch.zeros(n + 1, dtype=i64, device=dev),
         "payloads": torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=g),
         "user_headers": torch.zeros(16, dtype=torch.uint8, device=dev)}
    src = abi.UnpackedMessages(n, total, 16, *(a[k].data_ptr() for k in ORDER))
    o = {k: torch.empty_like(v) for k, v in a.items()}
    out = abi.UnpackedMessages(n, total, 16, *(o[k].data_ptr() for k in ORDER))
    d_idx = torch.empty(n, dtype=i64, device=dev)
    d_cnt = torch.full((1,), n, dtype=i64, device=dev)
    d_res = torch.zeros(ctypes.sizeof(abi.SelectResult), dtype=torch.uint8, device=dev)
    idx = torch.arange(n, device=dev)
    tenant = (idx % 100).to(torch.int32)
    v16 = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    v16[:, :4] = tenant.view(torch.uint8).view(n, 4)
    kinds = torch.full((n,), abi.KIND_INT32, dtype=torch.uint8, device=dev)
    lens = torch.full((n,), 4, dtype=torch.uint8, device=dev)
    col = abi.HeaderColumn(kinds.data_ptr(), lens.data_ptr(), None, v16.data_ptr())
    masks = {"keep_100": None, "keep_50": (idx % 2 == 1), "keep_1": (idx % 100 == 0), "header_clause": None}
    s = torch.cuda.current_stream().cuda_stream
    res = {"workload": name, "messages": n, "payload_bytes": total, "runs": runs}
    fixed = 16 + 8 + 8 + 8 + 8 + 4 + 4
    for case, m in masks.items():
        m8 = m.to(torch.uint8) if m is not None else None
        clauses = []
        if case == "header_clause":
            clauses = [abi.SelectClause.make(abi.SEL_HEADER, abi.OP_LT, (50).to_bytes(4, "little"), abi.KIND_INT32, col)]
            m = tenant < 50
        spec = abi.SelectSpec.make(clauses, m8.data_ptr() if m8 is not None else None)

        def run():
            rc = cx.select_messages_device(src, d_cnt.data_ptr(), spec, out, d_idx.data_ptr(), None,
                                           d_res.data_ptr(), s)
            assert rc == 0, rc

        med, lo_ms, hi_ms = events_ms(torch, run, runs)
        r = abi.SelectResult.from_buffer_copy(to_host(d_res).tobytes())
        want = idx if m is None else idx[m]
        kept_bytes = int(pls[want].to(i64).sum().item())
        assert r.error.kind == 0 and (r.examined, r.count, r.payload_bytes) == (n, want.numel(), kept_bytes), r.error
        assert torch.equal(d_idx[:r.count], want) and torch.equal(o["offsets"][:r.count], a["offsets"][want])
        if lo == hi:  # the kept payloads against a row gather
            assert torch.equal(o["payloads"][:kept_bytes].view(-1, lo), a["payloads"].view(n, lo)[want])
        else:
            assert torch.equal(o["payload_lengths"][:r.count], pls[want])
            j = int(want[-1].item())
            assert torch.equal(o["payloads"][kept_bytes - int(pls[j].item()):kept_bytes],
                               a["payloads"][int(starts[j].item()):int(starts[j + 1].item())])
        dst = torch.empty(max(kept_bytes, 1), dtype=torch.uint8, device=dev)
        cmed, clo, chi = events_ms(torch, lambda: dst[:kept_bytes].copy_(a["payloads"][:kept_bytes]), runs)
        # the flags read per message (mask or column), every kept array read and written, the scratch
        alg = n * (1 + 1 + (17 if clauses else 0)) + r.count * (2 * fixed + 16 + 3 * 8) + 2 * kept_bytes
        res[case] = {"kept": r.count, "kept_payload_bytes": kept_bytes, "ms": round(med, 4), "min_ms": round(lo_ms, 4),
                     "max_ms": round(hi_ms, 4), "algorithmic_bytes": alg,
                     "hbm_frac": round(alg / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                     "d2d_copy_of_kept_ms": round(cmed, 4), "ratio_to_copy": round(med / cmed, 3)}
        del dst
    # second yardstick at keep = 100 %: the unpack's byte-copy form over a record of the same bytes
    L = 256 + 48 * n + total
    rec = torch.empty(L, dtype=torch.uint8, device=dev)
    eres = torch.zeros(ctypes.sizeof(abi.EncodeResult), dtype=torch.uint8, device=dev)
    raw = abi.RawMessages(n, a["ids"].data_ptr(), a["origin_timestamps"].data_ptr(), a["payloads"].data_ptr(),
                          pls.data_ptr(), None, None)
    assert cx.encode_device(raw, 1, rec.data_ptr(), L, eres.data_ptr(), s) == 0
    pos = torch.empty(n, dtype=i64, device=dev)
    dres = torch.zeros(ctypes.sizeof(abi.DecodeResult), dtype=torch.uint8, device=dev)
    assert cx.decode_device(rec.data_ptr(), L, abi.INTEGRITY_VERIFY, pos.data_ptr(), n, dres.data_ptr(), s) == 0
    torch.cuda.synchronize()
    dr = abi.DecodeResult.from_buffer_copy(to_host(dres).tobytes())
    assert dr.error.kind == 0 and dr.frame_count == n, dr.error
    ures = torch.zeros(ctypes.sizeof(abi.UnpackResult), dtype=torch.uint8, device=dev)
    ub = abi.UnpackedMessages(n, total, 16, *(o[k].data_ptr() if k in ("payload_starts", "user_headers_starts",
                                                                        "payloads", "user_headers") else None
                                              for k in ORDER))

    def unpack_bytes():
        assert cx.unpack_device(rec.data_ptr(), L, pos.data_ptr(), dres.data_ptr(), ub, None, ures.data_ptr(), s) == 0

    umed, ulo, uhi = events_ms(torch, unpack_bytes, runs)
    ur = abi.UnpackResult.from_buffer_copy(to_host(ures).tobytes())
    assert ur.error.kind == 0 and ur.count == n and torch.equal(o["payloads"], a["payloads"]), ur.error
    res["unpack_byte_copy_form_ms"] = round(umed, 4)
    res["keep_100"]["ratio_to_unpack_byte_copy_form"] = round(res["keep_100"]["ms"] / umed, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from iggy_amd.codec import Codec
    if not torch.cuda.is_available():
        sys.exit("select_timing.py measures on an MI355X; no GPU found")
    torch.cuda.set_device(0)
    cx = Codec(0)
    # one explicit stream for the codec's work, the copies and the events (torch's default
    # stream is handle 0, which the C ABI reads as "the context's own stream")
    with torch.cuda.stream(torch.cuda.Stream()):
        assert torch.cuda.current_stream().cuda_stream != 0
        res = {"script": "scripts/select_timing.py", "device": torch.cuda.get_device_name(0),
               "c2": one(cx, "C2 arrays: 1,048,576 x 1 KiB", 1024, 1024, a.runs),
               "c3": one(cx, "C3 arrays: 1,048,576 msgs, payloads U[64,4096] B", 64, 4096, a.runs)}
    cx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

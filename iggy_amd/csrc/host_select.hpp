// host_select.hpp -- device-side select: the synchronous argument checks, scratch sizing
// and the enqueue of select.hip
//
// Part of the unity build of libiggy_codec.so: included by codec_api.hip, after the
// kernel translation units and the units before it (see codec_api.hip for the order).
#pragma once

namespace {

// [0, 256) control words | tile sums (kept, payload, user headers) | tile min / max |
// source index (8 B per message) | keep flags (1 B per message)
int ensure_select_scratch(iggy_codec_ctx *c, uint64_t messages) {
    messages = std::max<uint64_t>(messages, 1);
    if (messages <= c->sel_messages && c->sel.p) return 0;
    const uint64_t ntiles = messages / kSelTile + 2;
    if (c->sel.ensure(256 + ntiles * 32 + messages * 9)) return IGGY_ERR_DEVICE;
    c->sel_messages = messages;
    return 0;
}

SelScratch sscratch(iggy_codec_ctx *c) {
    const uint64_t ntiles = c->sel_messages / kSelTile + 2;
    SelScratch ss;
    ss.ctl = c->sel.as<uint64_t>(0);
    ss.tile_n = c->sel.as<uint64_t>(256);
    ss.tile_pl = c->sel.as<uint64_t>(256 + ntiles * 8);
    ss.tile_uh = c->sel.as<uint64_t>(256 + ntiles * 16);
    ss.tile_mm = c->sel.as<uint32_t>(256 + ntiles * 24);
    ss.sidx = c->sel.as<uint64_t>(256 + ntiles * 32);
    ss.flags = c->sel.as<uint8_t>(256 + ntiles * 32 + c->sel_messages * 8);
    ss.max_messages = c->sel_messages;
    return ss;
}

// an array wanted in out needs the same array in src, at another address
bool select_arrays_ok(const iggy_unpacked_messages *src, const iggy_unpacked_messages *out) {
    const void *const s[] = {src->ids, src->checksums, src->offsets, src->timestamps, src->origin_timestamps,
                             src->payload_lengths, src->user_headers_lengths, src->payload_starts,
                             src->user_headers_starts, src->payloads, src->user_headers};
    const void *const o[] = {out->ids, out->checksums, out->offsets, out->timestamps, out->origin_timestamps,
                             out->payload_lengths, out->user_headers_lengths, out->payload_starts,
                             out->user_headers_starts, out->payloads, out->user_headers};
    for (int k = 0; k < 11; ++k)
        if (o[k] && (!s[k] || s[k] == o[k])) return false;
    return !(out->payloads && !out->payload_starts) && !(out->user_headers && !out->user_headers_starts);
}

}  // namespace

extern "C" {

int iggy_codec_select_messages_device(iggy_codec_ctx *c, const iggy_unpacked_messages *src,
                                      const uint64_t *d_count, const iggy_select_spec *spec,
                                      const iggy_unpacked_messages *out, uint64_t *d_source_index,
                                      iggy_unpack_cursor *d_out_cursor, iggy_select_result *d_result,
                                      void *stream) {
    if (!c || !src || !d_count || !spec || !out || !d_result) return IGGY_ERR_INVALID_ARGUMENT;
    SelProgram prog;
    if (int r = sel_prepare(spec, src, prog)) return r;
    if (!select_arrays_ok(src, out)) return IGGY_ERR_INVALID_ARGUMENT;
    DevGuard dg(c->device);
    hipStream_t s = bind(c, stream);
    // (sized by iggy_codec_reserve; grown here only for a source larger than any before)
    if (int r = ensure_select_scratch(c, src->cap_messages)) return r;
    const SelScratch ss = sscratch(c);
    // grids from the capacities alone: the counts stay on the device
    const uint64_t wgs = (uint64_t)c->ncu * 8;
    const uint32_t gtiles =
        (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((src->cap_messages + kSelTile - 1) / kSelTile, wgs));
    hipLaunchKernelGGL(k_sel_flags, dim3(gtiles), dim3(256), 0, s, *src, d_count, prog, ss);
    hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(256), 0, s, *src, d_count, *out, d_out_cursor, ss, d_result);
    hipLaunchKernelGGL(k_sel_fields, dim3(gtiles), dim3(256), 0, s, *src, *out, d_source_index, ss);
    if (out->payloads) {
        const uint64_t spans = std::min(out->cap_payload_bytes, src->cap_payload_bytes) / kUpSpan + 2;
        hipLaunchKernelGGL(k_sel_copy<true>, dim3((uint32_t)std::min(spans, wgs)), dim3(256), 0, s,
                           (const uint8_t *)src->payloads, (const uint64_t *)src->payload_starts,
                           (const uint64_t *)out->payload_starts, out->payloads, 0u, ss);
    }
    if (out->user_headers) {
        const uint64_t spans = std::min(out->cap_user_headers_bytes, src->cap_user_headers_bytes) / kUpSpan + 2;
        hipLaunchKernelGGL(k_sel_copy<true>, dim3((uint32_t)std::min(spans, wgs)), dim3(256), 0, s,
                           (const uint8_t *)src->user_headers, (const uint64_t *)src->user_headers_starts,
                           (const uint64_t *)out->user_headers_starts, out->user_headers, 1u, ss);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

}  // extern "C"

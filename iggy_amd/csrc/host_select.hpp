// host_select.hpp -- device-side select: the synchronous argument checks, scratch sizing
// and the enqueue of select.hip
//
// Part of the unity build of libiggy_codec.so: included by codec_api.hip, after the
// kernel translation units and the units before it (see codec_api.hip for the order).
#pragma once

namespace {

SelScratch select_layout(Carve &cv, uint64_t messages) {
    const uint64_t ntiles = messages / kSelTile + 2;
    SelScratch ss;
    ss.ctl = cv.take<uint64_t>(256);  // (control words: 8 used)
    ss.tile_n = cv.take<uint64_t>(ntiles * 8);
    ss.tile_pl = cv.take<uint64_t>(ntiles * 8);
    ss.tile_uh = cv.take<uint64_t>(ntiles * 8);
    ss.tile_mm = cv.take<uint32_t>(ntiles * 8);
    ss.sidx = cv.take<uint64_t>(messages * 8);
    ss.flags = cv.take<uint8_t>(messages);
    ss.max_messages = messages;
    return ss;
}

int ensure_select_scratch(iggy_codec_ctx *c, uint64_t messages) {
    messages = std::max<uint64_t>(messages, 1);
    if (messages <= c->sel_messages && c->sel.p) return 0;
    Carve size{nullptr};
    select_layout(size, messages);
    if (c->sel.ensure(size.at)) return IGGY_ERR_DEVICE;
    c->sel_messages = messages;
    return 0;
}

SelScratch sscratch(iggy_codec_ctx *c) {
    Carve cv{c->sel.as<uint8_t>()};
    return select_layout(cv, c->sel_messages);
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
    using Source = SoaIndexedSource<true>;
    launch_copies(s, wgs, *out, ss.ctl, Source{src->payloads, src->payload_starts, ss.sidx},
                  std::min(out->cap_payload_bytes, src->cap_payload_bytes),
                  Source{src->user_headers, src->user_headers_starts, ss.sidx},
                  std::min(out->cap_user_headers_bytes, src->cap_user_headers_bytes));
    HIP_OK(hipGetLastError());
    return 0;
}

}  // extern "C"

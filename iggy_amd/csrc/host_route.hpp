// host_route.hpp -- device-side route: the synchronous argument checks, scratch sizing and
// the enqueue of route.hip
//
// Part of the unity build of libiggy_codec.so: included by codec_api.hip, after the
// kernel translation units and the units before it (see codec_api.hip for the order).
#pragma once

namespace {

RouteScratch route_layout(Carve &cv, uint64_t messages) {
    const uint64_t nt = messages / kRtTile + 2, nd = messages / kRtDTile + 2;
    RouteScratch rs;
    rs.ctl = cv.take<uint64_t>(256);  // (control words: 8 used)
    rs.tile_pl = cv.take<uint64_t>(nt * 8);
    rs.tile_uh = cv.take<uint64_t>(nt * 8);
    rs.dtile_pl = cv.take<uint64_t>(nd * 8);
    rs.dtile_uh = cv.take<uint64_t>(nd * 8);
    rs.hist = cv.take<uint32_t>(nt * kRtParts * 4);
    rs.sidx = cv.take<uint64_t>(messages * 8);
    rs.dlens = cv.take<uint2>(messages * 8);
    rs.part = cv.take<uint16_t>(messages * 2);
    rs.max_messages = messages;
    return rs;
}

int ensure_route_scratch(iggy_codec_ctx *c, uint64_t messages) {
    messages = std::max<uint64_t>(messages, 1);
    if (messages <= c->rt_messages && c->rt.p) return 0;
    Carve size{nullptr};
    route_layout(size, messages);
    if (c->rt.ensure(size.at)) return IGGY_ERR_DEVICE;
    c->rt_messages = messages;
    return 0;
}

RouteScratch rscratch(iggy_codec_ctx *c) {
    Carve cv{c->rt.as<uint8_t>()};
    return route_layout(cv, c->rt_messages);
}

}  // namespace

extern "C" {

int iggy_codec_route_messages_device(iggy_codec_ctx *c, const iggy_unpacked_messages *src,
                                     const uint64_t *d_count, const iggy_route_spec *spec,
                                     const iggy_unpacked_messages *out, uint64_t *d_partition_first,
                                     uint64_t *d_partition_payload_first, uint64_t *d_partition_user_headers_first,
                                     uint32_t *d_partition_of, uint64_t *d_source_index,
                                     iggy_route_result *d_result, void *stream) {
    if (!c || !src || !d_count || !spec || !d_result || !d_partition_first) return IGGY_ERR_INVALID_ARGUMENT;
    RouteProgram prog;
    if (int r = route_prepare(spec, src, prog)) return r;
    if (out) {
        if (!select_arrays_ok(src, out)) return IGGY_ERR_INVALID_ARGUMENT;
        if ((d_partition_payload_first && !out->payload_starts) ||
            (d_partition_user_headers_first && !out->user_headers_starts))
            return IGGY_ERR_INVALID_ARGUMENT;
    } else if (d_partition_payload_first || d_partition_user_headers_first || d_source_index) {
        return IGGY_ERR_INVALID_ARGUMENT;
    }
    if (src->cap_messages >> 32) return IGGY_ERR_INVALID_ARGUMENT;  // (the destination bases are u32)
    DevGuard dg(c->device);
    hipStream_t s = bind(c, stream);
    // (sized by iggy_codec_reserve; grown here only for a source larger than any before)
    if (int r = ensure_route_scratch(c, src->cap_messages)) return r;
    const RouteScratch rs = rscratch(c);
    const iggy_unpacked_messages o = out ? *out : iggy_unpacked_messages{};
    const uint32_t has_out = out ? 1u : 0u;
    // grids from the capacities alone: the counts stay on the device
    const uint64_t wgs = (uint64_t)c->ncu * 8;
    const uint32_t gtiles =
        (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((src->cap_messages + kRtTile - 1) / kRtTile, wgs));
    hipLaunchKernelGGL(k_route_keys, dim3(gtiles), dim3(256), 0, s, *src, d_count, prog, rs);
    hipLaunchKernelGGL(k_route_scan, dim3(1), dim3(256), 0, s, *src, d_count, prog.partitions, o, has_out,
                       d_partition_first, rs, d_result);
    if (out || d_partition_of)
        hipLaunchKernelGGL(k_route_fields, dim3(gtiles), dim3(256), 0, s, *src, o, has_out, prog.partitions,
                           d_partition_of, d_source_index, rs);
    if (out) {
        const uint64_t m = std::min(out->cap_messages, src->cap_messages);
        const uint32_t gd = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((m + kRtDTile - 1) / kRtDTile, wgs));
        hipLaunchKernelGGL(k_route_dscan, dim3(1), dim3(256), 0, s, rs);
        hipLaunchKernelGGL(k_route_starts, dim3(gd), dim3(256), 0, s, o, prog.partitions,
                           (const uint64_t *)d_partition_first, d_partition_payload_first,
                           d_partition_user_headers_first, rs);
        using Source = SoaIndexedSource<false>;
        launch_copies(s, wgs, *out, rs.ctl, Source{src->payloads, src->payload_starts, rs.sidx},
                      std::min(out->cap_payload_bytes, src->cap_payload_bytes),
                      Source{src->user_headers, src->user_headers_starts, rs.sidx},
                      std::min(out->cap_user_headers_bytes, src->cap_user_headers_bytes));
    }
    HIP_OK(hipGetLastError());
    return 0;
}

}  // extern "C"

// host_route.hpp -- device-side route: the synchronous argument checks, scratch sizing and
// the enqueue of route.hip
//
// Part of the unity build of libiggy_codec.so: included by codec_api.hip, after the
// kernel translation units and the units before it (see codec_api.hip for the order).
#pragma once

namespace {

// [0, 256) control words | source tile byte sums (2 x 8 B per tile of 2048) | destination
// tile byte sums (2 x 8 B per 1024) | partition counts (256 x 4 B per tile) | source index
// (8 B per message) | lengths in destination order (8 B) | partition (2 B)
uint64_t route_tiles(uint64_t messages) { return messages / kRtTile + 2; }
uint64_t route_dtiles(uint64_t messages) { return messages / kRtDTile + 2; }

int ensure_route_scratch(iggy_codec_ctx *c, uint64_t messages) {
    messages = std::max<uint64_t>(messages, 1);
    if (messages <= c->rt_messages && c->rt.p) return 0;
    const uint64_t nt = route_tiles(messages), nd = route_dtiles(messages);
    if (c->rt.ensure(256 + nt * 16 + nd * 16 + nt * kRtParts * 4 + messages * 18)) return IGGY_ERR_DEVICE;
    c->rt_messages = messages;
    return 0;
}

RouteScratch rscratch(iggy_codec_ctx *c) {
    const uint64_t nt = route_tiles(c->rt_messages), nd = route_dtiles(c->rt_messages), m = c->rt_messages;
    RouteScratch rs;
    uint64_t at = 0;
    rs.ctl = c->rt.as<uint64_t>(at), at += 256;
    rs.tile_pl = c->rt.as<uint64_t>(at), at += nt * 8;
    rs.tile_uh = c->rt.as<uint64_t>(at), at += nt * 8;
    rs.dtile_pl = c->rt.as<uint64_t>(at), at += nd * 8;
    rs.dtile_uh = c->rt.as<uint64_t>(at), at += nd * 8;
    rs.hist = c->rt.as<uint32_t>(at), at += nt * kRtParts * 4;
    rs.sidx = c->rt.as<uint64_t>(at), at += m * 8;
    rs.dlens = c->rt.as<uint2>(at), at += m * 8;
    rs.part = c->rt.as<uint16_t>(at);
    rs.max_messages = m;
    return rs;
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
        SelScratch ss{};  // the copy reads the control words and the source index alone
        ss.ctl = rs.ctl;
        ss.sidx = rs.sidx;
        ss.max_messages = rs.max_messages;
        if (out->payloads) {
            const uint64_t spans = std::min(out->cap_payload_bytes, src->cap_payload_bytes) / kUpSpan + 2;
            hipLaunchKernelGGL(k_sel_copy<false>, dim3((uint32_t)std::min(spans, wgs)), dim3(256), 0, s,
                               (const uint8_t *)src->payloads, (const uint64_t *)src->payload_starts,
                               (const uint64_t *)out->payload_starts, out->payloads, 0u, ss);
        }
        if (out->user_headers) {
            const uint64_t spans = std::min(out->cap_user_headers_bytes, src->cap_user_headers_bytes) / kUpSpan + 2;
            hipLaunchKernelGGL(k_sel_copy<false>, dim3((uint32_t)std::min(spans, wgs)), dim3(256), 0, s,
                               (const uint8_t *)src->user_headers, (const uint64_t *)src->user_headers_starts,
                               (const uint64_t *)out->user_headers_starts, out->user_headers, 1u, ss);
        }
    }
    HIP_OK(hipGetLastError());
    return 0;
}

}  // extern "C"

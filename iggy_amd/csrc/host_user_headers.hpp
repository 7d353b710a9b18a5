// host_user_headers.hpp -- user-header validation and key columns: the synchronous
// argument checks and the enqueue of user_headers.hip
//
// Part of the unity build of libiggy_codec.so: included by codec_api.hip, after the
// kernel translation units and the units before it (see codec_api.hip for the order).
#pragma once

namespace {

// the request as the kernel takes it (keys by value with the launch); IGGY_ERR_INVALID_ARGUMENT
// for what the header says is refused synchronously
int uh_request(const iggy_header_columns *q, UhKeys &keys, UhOut &o) {
    if (!q || q->nkeys > IGGY_HEADER_MAX_KEYS) return IGGY_ERR_INVALID_ARGUMENT;
    memset(&keys, 0, sizeof keys);
    uint32_t used = 0;
    for (uint32_t k = 0; k < q->nkeys; ++k) {
        const iggy_header_key &key = q->keys[k];
        if (!uh_key_ok(key.kind, key.length) || used + key.length > IGGY_HEADER_MAX_KEY_BYTES)
            return IGGY_ERR_INVALID_ARGUMENT;
        keys.kind[k] = key.kind;
        keys.len[k] = key.length;
        keys.off[k] = (uint16_t)used;
        memcpy(keys.bytes + used, key.bytes, key.length);
        used += key.length;
    }
    keys.nkeys = q->nkeys;
    o.cap = q->cap_messages;
    for (uint32_t k = 0; k < IGGY_HEADER_MAX_KEYS; ++k) o.col[k] = k < q->nkeys ? q->columns[k] : iggy_header_column{};
    o.status = q->status;
    o.pairs = q->pairs;
    return 0;
}

int uh_enqueue(iggy_codec_ctx *c, const UhSrc &in, uint64_t max_frames, uint64_t tiles_hint, const UhKeys &keys,
               const UhOut &o, iggy_header_columns_result *d_result, void *stream) {
    DevGuard dg(c->device);
    hipStream_t s = bind(c, stream);
    if (c->uh.ensure(256)) return IGGY_ERR_DEVICE;  // the control words
    uint64_t *ctl = c->uh.as<uint64_t>(0);
    // the grid from the record's length (the hint) alone: the count stays on the device, and
    // the tiles are handed out by a counter, so any count is served by any grid
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles_hint, (uint64_t)c->ncu * 3));
    hipLaunchKernelGGL(k_uh_init, dim3(1), dim3(64), 0, s, in, o.cap, max_frames, d_result, ctl);
    hipLaunchKernelGGL(k_uh_columns, dim3(grid), dim3(256), 0, s, in, keys, o, d_result, ctl);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int iggy_codec_user_headers_device(iggy_codec_ctx *c, const uint8_t *d_record, uint64_t len,
                                   const uint64_t *d_frame_pos, const iggy_decode_result *d_decode,
                                   const iggy_header_columns *q, iggy_header_columns_result *d_result,
                                   void *stream) {
    if (!c || !d_record || !d_decode || !q || !d_result || len < kHdr) return IGGY_ERR_INVALID_ARGUMENT;
    if (!d_frame_pos && len > kHdr) return IGGY_ERR_INVALID_ARGUMENT;
    UhKeys keys;
    UhOut o;
    if (int r = uh_request(q, keys, o)) return r;
    const uint64_t max_frames = unpack_max_frames(len);
    UhSrc in{};
    in.rec = d_record;
    in.pos = d_frame_pos;
    in.dec = d_decode;
    in.len = len;
    return uh_enqueue(c, in, max_frames, (max_frames + kUhTile - 1) / kUhTile, keys, o, d_result, stream);
}

int iggy_codec_user_headers_arrays_device(iggy_codec_ctx *c, const uint8_t *d_user_headers,
                                          const uint64_t *d_user_headers_starts, const uint64_t *d_count,
                                          uint64_t cap_messages_hint, const iggy_header_columns *q,
                                          iggy_header_columns_result *d_result, void *stream) {
    if (!c || !d_user_headers_starts || !d_count || !q || !d_result) return IGGY_ERR_INVALID_ARGUMENT;
    UhKeys keys;
    UhOut o;
    if (int r = uh_request(q, keys, o)) return r;
    UhSrc in{};
    in.blob = d_user_headers;
    in.starts = d_user_headers_starts;
    in.count = d_count;
    return uh_enqueue(c, in, 0, cap_messages_hint / kUhTile + 1, keys, o, d_result, stream);
}

}  // extern "C"

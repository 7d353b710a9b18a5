// host_unpack.hpp -- consumer unpack: scratch sizing and the enqueue of unpack.hip
//
// Part of the unity build of libiggy_codec.so: included by codec_api.hip, after the
// kernel translation units and the units before it (see codec_api.hip for the order).
#pragma once

namespace {

// frames a record of `len` bytes can hold (48-B headers tiling its blob)
inline uint64_t unpack_max_frames(uint64_t len) { return len > kHdr ? (len - kHdr) / kFrameHdr + 1 : 1; }

// A scratch buffer carved front to back, so that a stage writes its layout once: take() is
// the next sub-array, `at` the bytes taken so far. With p = NULL only `at` means anything:
// the size to allocate.
struct Carve {
    uint8_t *p;
    uint64_t at = 0;
    template <class T> T *take(uint64_t bytes) {
        T *r = p ? (T *)(p + at) : nullptr;
        at += bytes;
        return r;
    }
};

UnpackScratch unpack_layout(Carve &cv, uint64_t frames) {
    const uint64_t ntiles = frames / kUpTile + 2;
    UnpackScratch us;
    us.ctl = cv.take<uint64_t>(256);  // (control words: 8 used)
    us.tile_pl = cv.take<uint64_t>(ntiles * 8);
    us.tile_uh = cv.take<uint64_t>(ntiles * 8);
    us.tile_mm = cv.take<uint32_t>(ntiles * 8);
    us.lens = cv.take<uint2>(frames * 8);
    us.max_frames = frames;
    return us;
}

int ensure_unpack_scratch(iggy_codec_ctx *c, uint64_t len) {
    const uint64_t frames = unpack_max_frames(len);
    if (frames <= c->up_frames && c->up.p) return 0;
    Carve size{nullptr};
    unpack_layout(size, frames);
    if (c->up.ensure(size.at)) return IGGY_ERR_DEVICE;
    c->up_frames = frames;
    return 0;
}

UnpackScratch uscratch(iggy_codec_ctx *c) {
    Carve cv{c->up.as<uint8_t>()};
    return unpack_layout(cv, c->up_frames);
}

// The two byte-copy launches of a stage, payloads then user headers. pl / uh: their
// sources; bytes_pl / bytes_uh: the most bytes each launch can have to move, which sizes
// its grid (the totals stay on the device); ctl: the stage's control words.
template <class Source>
void launch_copies(hipStream_t s, uint64_t wgs, const iggy_unpacked_messages &out, const uint64_t *ctl,
                   const Source &pl, uint64_t bytes_pl, const Source &uh, uint64_t bytes_uh) {
    if (out.payloads)
        hipLaunchKernelGGL(k_soa_copy<Source>, dim3((uint32_t)std::min(bytes_pl / kSoaSpan + 2, wgs)), dim3(256), 0, s,
                           pl, (const uint64_t *)out.payload_starts, out.payloads, 0u, ctl);
    if (out.user_headers)
        hipLaunchKernelGGL(k_soa_copy<Source>, dim3((uint32_t)std::min(bytes_uh / kSoaSpan + 2, wgs)), dim3(256), 0, s,
                           uh, (const uint64_t *)out.user_headers_starts, out.user_headers, 1u, ctl);
}

}  // namespace

extern "C" {

int iggy_codec_unpack_batch_device(iggy_codec_ctx *c, const uint8_t *d_record, uint64_t len,
                                   const uint64_t *d_frame_pos, const iggy_decode_result *d_decode,
                                   const iggy_unpacked_messages *out, iggy_unpack_cursor *d_cursor,
                                   iggy_unpack_result *d_result, void *stream) {
    if (!c || !d_record || !d_decode || !out || !d_result || len < kHdr) return IGGY_ERR_INVALID_ARGUMENT;
    if ((out->payloads && !out->payload_starts) || (out->user_headers && !out->user_headers_starts))
        return IGGY_ERR_INVALID_ARGUMENT;
    const uint64_t max_frames = unpack_max_frames(len);
    if (!d_frame_pos && len > kHdr) return IGGY_ERR_INVALID_ARGUMENT;
    DevGuard dg(c->device);
    hipStream_t s = bind(c, stream);
    // (sized by iggy_codec_reserve; grown here only for a record larger than any before)
    if (int r = ensure_unpack_scratch(c, len)) return r;
    const UnpackScratch us = uscratch(c);
    // grids from the record's length and the capacities alone: the count stays on the device
    const uint64_t wgs = (uint64_t)c->ncu * 8;
    const uint32_t gtiles = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((max_frames + kUpTile - 1) / kUpTile, wgs));
    hipLaunchKernelGGL(k_unpack_fields, dim3(gtiles), dim3(256), 0, s, d_record, len, d_frame_pos, d_decode, *out,
                       (const iggy_unpack_cursor *)d_cursor, us);
    hipLaunchKernelGGL(k_unpack_scan, dim3(1), dim3(256), 0, s, len, d_decode, *out, d_cursor, us, d_result);
    if (out->payload_starts || out->user_headers_starts)
        hipLaunchKernelGGL(k_unpack_starts, dim3(gtiles), dim3(256), 0, s, *out, us);
    const uint64_t blob = len - kHdr;
    if (blob)
        launch_copies(s, wgs, *out, us.ctl, SoaRecordSource{d_record, d_frame_pos, us.lens, 0u},
                      std::min(out->cap_payload_bytes, blob), SoaRecordSource{d_record, d_frame_pos, us.lens, 1u},
                      std::min(out->cap_user_headers_bytes, blob));
    HIP_OK(hipGetLastError());
    return 0;
}

}  // extern "C"

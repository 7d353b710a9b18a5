// unpack.hip — consumer unpack: a verified device-resident record back into the
// struct-of-arrays the encoder takes (iggy_raw_messages), the GPU form of
// PolledMessages::messages_from_batches (core/common/src/types/message/
// polled_messages.rs:95-150; PolledBatchesIterator, core/binary_protocol/src/responses/
// messages/poll_messages.rs:132-165; RawMessage, requests/messages/send_messages.rs:37-42).
//
//  k_unpack_fields : one thread per frame: the 48-B header at its (arbitrary) address,
//                    the fixed-width arrays with coalesced stores, both lengths into
//                    scratch, and per 256-frame tile the two length sums and the
//                    min / max payload length.
//  k_unpack_scan   : one WG: exclusive scan of the tile sums (u64), the cursor's bases,
//                    the capacity verdict, the result, the cursor's advance.
//  k_unpack_starts : per tile the exclusive scan of the staged lengths + tile offset +
//                    base -> payload_starts / user_headers_starts (entry [count] = end).
//  k_soa_copy<SoaRecordSource> (soa_common.hpp): the byte copy the select and the route
//                    share, reading each message at its frame's position in the record.
//
// The scans, the placement behind the cursor and the control words are soa_common.hpp's.
// Every kernel reads the message count from the decode's device-resident result; the
// host sizes the grids from the record's length and the capacities alone.
#include "soa_common.hpp"

namespace iggy {

constexpr uint32_t kUpTile = 256;  // frames per tile (one per thread)

struct UnpackScratch {
    uint64_t *ctl;        // [8] kSoa* words, kSoaAux = the record's batch_length (wide loads stay inside it)
    uint64_t *tile_pl;    // [ntiles] tile sums -> tile offsets after the scan
    uint64_t *tile_uh;    // [ntiles]
    uint32_t *tile_mm;    // [2 * ntiles] min, max payload length
    uint2 *lens;          // [max_frames] payload_length, user_headers_length
    uint64_t max_frames;  // frames the scratch holds (the record's length bounds them)
};

// the decode's verdict as the unpack takes it: its own error, or InvalidArgument for a
// result that is not final or cannot belong to a record of `len` bytes
__device__ __forceinline__ uint32_t unpack_gate(const iggy_decode_result *d, uint64_t len, uint64_t max_frames) {
    if (d->error.kind != IGGY_OK) return d->error.kind;
    if (d->status != kStatusDone || d->frame_count > max_frames || d->header.batch_length < kHdr ||
        d->header.batch_length > len)
        return IGGY_ERR_INVALID_ARGUMENT;
    return IGGY_OK;
}

__global__ __launch_bounds__(256) void k_unpack_fields(const uint8_t *rec, uint64_t len, const uint64_t *pos,
                                                       const iggy_decode_result *d, iggy_unpacked_messages o,
                                                       const iggy_unpack_cursor *cur, UnpackScratch us) {
    __shared__ uint64_t s_pl[256], s_uh[256];
    __shared__ uint32_t s_mn[256], s_mx[256];
    if (unpack_gate(d, len, us.max_frames) != IGGY_OK) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t n = d->frame_count;
    const uint64_t first = cur ? cur->messages : 0;
    const uint64_t base_offset = d->header.base_offset, base_ts = d->header.base_timestamp,
                   origin = d->header.origin_timestamp;
    const uint64_t ntiles = (n + kUpTile - 1) / kUpTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i = t * kUpTile + tid;
        uint32_t pl = 0, uh = 0;
        if (i < n) {
            const uint8_t *f = rec + kHdr + pos[i];
            uh = ld32_any(f + 32);
            pl = ld32_any(f + 36);
            us.lens[i] = make_uint2(pl, uh);
            const uint64_t j = first + i;
            // (a capacity violation is the scan's verdict; until then nothing may land past a capacity)
            if (j >= first && j < o.cap_messages) {
                if (o.ids) {
                    o.ids[2 * j] = ld64_any(f + 8);
                    o.ids[2 * j + 1] = ld64_any(f + 16);
                }
                if (o.checksums) o.checksums[j] = ld64_any(f);
                if (o.offsets) o.offsets[j] = base_offset + ld32_any(f + 24);  // wrapping, as k_poll_fill
                if (o.timestamps) o.timestamps[j] = base_ts;                   // flat per batch
                if (o.origin_timestamps) o.origin_timestamps[j] = origin + ld32_any(f + 28);
                if (o.payload_lengths) o.payload_lengths[j] = pl;
                if (o.user_headers_lengths) o.user_headers_lengths[j] = uh;
            }
        }
        s_pl[tid] = pl;
        s_uh[tid] = uh;
        s_mn[tid] = i < n ? pl : 0xFFFFFFFFu;
        s_mx[tid] = pl;
        __syncthreads();
        soa_reduce<true>(tid, s_mn, s_mx, s_pl, s_uh);
        if (tid == 0) {
            us.tile_pl[t] = s_pl[0];
            us.tile_uh[t] = s_uh[0];
            us.tile_mm[2 * t] = s_mn[0];
            us.tile_mm[2 * t + 1] = s_mx[0];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_unpack_scan(uint64_t len, const iggy_decode_result *d,
                                                     iggy_unpacked_messages o, iggy_unpack_cursor *cur,
                                                     UnpackScratch us, iggy_unpack_result *res) {
    const uint32_t tid = threadIdx.x;
    if (unpack_gate(d, len, us.max_frames) != IGGY_OK) {
        if (tid == 0) {
            iggy_unpack_result r{};
            if (d->error.kind != IGGY_OK) r.error = d->error;
            else r.error.kind = IGGY_ERR_INVALID_ARGUMENT;
            r.first_message = cur ? cur->messages : 0;
            *res = r;
            us.ctl[kSoaOk] = 0;
        }
        return;
    }
    const uint64_t n = d->frame_count;
    uint64_t *const tiles[2] = {us.tile_pl, us.tile_uh};
    const SoaTotals<2> tot = soa_tile_offsets<true>(tid, (n + kUpTile - 1) / kUpTile, tiles, us.tile_mm);
    if (tid != 0) return;
    const SoaPlacement p = soa_place(cur, o, n, tot.sum[0], tot.sum[1]);
    iggy_unpack_result r{};
    r.first_message = p.first;
    if (p.fits) {
        r.count = n;
        r.payload_bytes = tot.sum[0];
        r.user_headers_bytes = tot.sum[1];
        r.min_payload_length = n ? tot.mn : 0;
        r.max_payload_length = tot.mx;
    } else {
        r.error = soa_capacity_error(p);
    }
    *res = r;
    soa_publish(us.ctl, cur, p, n, tot.sum[0], tot.sum[1], d->header.batch_length);
}

__global__ __launch_bounds__(256) void k_unpack_starts(iggy_unpacked_messages o, UnpackScratch us) {
    __shared__ uint64_t s_pl[256], s_uh[256];
    if (!us.ctl[kSoaOk]) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t first = us.ctl[kSoaFirst], n = us.ctl[kSoaCount];
    const uint64_t base_pl = us.ctl[kSoaBasePl], base_uh = us.ctl[kSoaBaseUh];
    const uint64_t ntiles = (n + kUpTile - 1) / kUpTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i = t * kUpTile + tid;
        const uint2 v = i < n ? us.lens[i] : make_uint2(0, 0);
        s_pl[tid] = v.x;
        s_uh[tid] = v.y;
        __syncthreads();
        soa_scan(tid, s_pl, s_uh);
        if (i < n) {
            if (o.payload_starts) o.payload_starts[first + i] = base_pl + us.tile_pl[t] + s_pl[tid] - v.x;
            if (o.user_headers_starts) o.user_headers_starts[first + i] = base_uh + us.tile_uh[t] + s_uh[tid] - v.y;
        }
        __syncthreads();
    }
    if (blockIdx.x == 0 && tid == 0) {  // the end entry, shared with the next chained record
        if (o.payload_starts) o.payload_starts[first + n] = base_pl + us.ctl[kSoaTotPl];
        if (o.user_headers_starts) o.user_headers_starts[first + n] = base_uh + us.ctl[kSoaTotUh];
    }
}

}  // namespace iggy


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
//  k_unpack_copy   : work split by OUTPUT bytes: a workgroup owns 32 KiB spans of the
//                    destination (16-B aligned to the destination address), finds the
//                    messages under a span by binary search in the starts, and moves
//                    one 16-B destination chunk per thread: an aligned store of an
//                    unaligned load where the chunk lies inside one message, byte-wise
//                    where messages (or the array's ends) meet inside the chunk, so a
//                    thread only ever writes bytes of the array's own range.
//
// Every kernel reads the message count from the decode's device-resident result; the
// host sizes the grids from the record's length and the capacities alone.
#include "codec_common.hpp"

namespace iggy {

constexpr uint32_t kUpTile = 256;                  // frames per tile (one per thread)
constexpr uint32_t kUpSpan = 32u << 10;            // destination bytes per copy span
constexpr uint32_t kUpChunks = kUpSpan / 16;       // 16-B chunks per span
constexpr uint32_t kUpStage = 1024;                // starts of a span staged in LDS (else read in place)
// control words published by k_unpack_scan for the kernels after it
constexpr uint32_t kUpOk = 0, kUpFirst = 1, kUpCount = 2, kUpBasePl = 3, kUpBaseUh = 4, kUpTotPl = 5, kUpTotUh = 6,
                   kUpRecLen = 7;  // the record's batch_length (wide loads stay inside it)

struct UnpackScratch {
    uint64_t *ctl;        // [8] kUp* words
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
        for (uint32_t k = 128; k > 0; k >>= 1) {
            if (tid < k) {
                s_pl[tid] += s_pl[tid + k];
                s_uh[tid] += s_uh[tid + k];
                s_mn[tid] = min(s_mn[tid], s_mn[tid + k]);
                s_mx[tid] = max(s_mx[tid], s_mx[tid + k]);
            }
            __syncthreads();
        }
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
    __shared__ uint64_t s_pl[256], s_uh[256];
    __shared__ uint32_t s_mn[256], s_mx[256];
    __shared__ uint64_t carry_pl, carry_uh;
    __shared__ uint32_t carry_mn, carry_mx;
    const uint32_t tid = threadIdx.x;
    const uint64_t first = cur ? cur->messages : 0;
    const uint32_t gate = unpack_gate(d, len, us.max_frames);
    if (gate != IGGY_OK) {
        if (tid == 0) {
            iggy_unpack_result r{};
            if (d->error.kind != IGGY_OK) r.error = d->error;
            else r.error.kind = IGGY_ERR_INVALID_ARGUMENT;
            r.first_message = first;
            *res = r;
            us.ctl[kUpOk] = 0;
        }
        return;
    }
    const uint64_t n = d->frame_count;
    const uint64_t ntiles = (n + kUpTile - 1) / kUpTile;
    if (tid == 0) { carry_pl = 0; carry_uh = 0; carry_mn = 0xFFFFFFFFu; carry_mx = 0; }
    __syncthreads();
    for (uint64_t t0 = 0; t0 < ntiles; t0 += 256) {
        const uint64_t t = t0 + tid;
        const uint64_t vpl = t < ntiles ? us.tile_pl[t] : 0;
        const uint64_t vuh = t < ntiles ? us.tile_uh[t] : 0;
        s_pl[tid] = vpl;
        s_uh[tid] = vuh;
        s_mn[tid] = t < ntiles ? us.tile_mm[2 * t] : 0xFFFFFFFFu;
        s_mx[tid] = t < ntiles ? us.tile_mm[2 * t + 1] : 0;
        __syncthreads();
        for (uint32_t k = 1; k < 256; k <<= 1) {  // inclusive scan (Hillis-Steele in LDS, as k_enc_scan)
            const uint64_t a = tid >= k ? s_pl[tid - k] : 0;
            const uint64_t b = tid >= k ? s_uh[tid - k] : 0;
            __syncthreads();
            s_pl[tid] += a;
            s_uh[tid] += b;
            __syncthreads();
        }
        if (t < ntiles) {
            us.tile_pl[t] = carry_pl + s_pl[tid] - vpl;
            us.tile_uh[t] = carry_uh + s_uh[tid] - vuh;
        }
        for (uint32_t k = 128; k > 0; k >>= 1) {
            if (tid < k) {
                s_mn[tid] = min(s_mn[tid], s_mn[tid + k]);
                s_mx[tid] = max(s_mx[tid], s_mx[tid + k]);
            }
            __syncthreads();
        }
        if (tid == 0) {
            carry_pl += s_pl[255];
            carry_uh += s_uh[255];
            carry_mn = min(carry_mn, s_mn[0]);
            carry_mx = max(carry_mx, s_mx[0]);
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const uint64_t base_pl = cur ? cur->payload_bytes : 0, base_uh = cur ? cur->user_headers_bytes : 0;
    const uint64_t need_m = sat_add(first, n), need_pl = sat_add(base_pl, carry_pl), need_uh = sat_add(base_uh, carry_uh);
    const bool fits = need_m <= o.cap_messages && (!o.payloads || need_pl <= o.cap_payload_bytes) &&
                      (!o.user_headers || need_uh <= o.cap_user_headers_bytes);
    iggy_unpack_result r{};
    r.first_message = first;
    if (fits) {
        r.count = n;
        r.payload_bytes = carry_pl;
        r.user_headers_bytes = carry_uh;
        r.min_payload_length = n ? carry_mn : 0;
        r.max_payload_length = carry_mx;
        if (cur) {
            cur->messages = need_m;
            cur->payload_bytes = need_pl;
            cur->user_headers_bytes = need_uh;
        }
    } else {
        r.error.kind = IGGY_ERR_CAPACITY;
        r.error.a = need_m;
        r.error.b = need_pl;
        r.error.c = need_uh;
    }
    *res = r;
    us.ctl[kUpOk] = fits ? 1 : 0;
    us.ctl[kUpFirst] = first;
    us.ctl[kUpCount] = n;
    us.ctl[kUpBasePl] = base_pl;
    us.ctl[kUpBaseUh] = base_uh;
    us.ctl[kUpTotPl] = carry_pl;
    us.ctl[kUpTotUh] = carry_uh;
    us.ctl[kUpRecLen] = d->header.batch_length;
}

__global__ __launch_bounds__(256) void k_unpack_starts(iggy_unpacked_messages o, UnpackScratch us) {
    __shared__ uint64_t s_pl[256], s_uh[256];
    if (!us.ctl[kUpOk]) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t first = us.ctl[kUpFirst], n = us.ctl[kUpCount];
    const uint64_t base_pl = us.ctl[kUpBasePl], base_uh = us.ctl[kUpBaseUh];
    const uint64_t ntiles = (n + kUpTile - 1) / kUpTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i = t * kUpTile + tid;
        const uint2 v = i < n ? us.lens[i] : make_uint2(0, 0);
        s_pl[tid] = v.x;
        s_uh[tid] = v.y;
        __syncthreads();
        for (uint32_t k = 1; k < 256; k <<= 1) {
            const uint64_t a = tid >= k ? s_pl[tid - k] : 0;
            const uint64_t b = tid >= k ? s_uh[tid - k] : 0;
            __syncthreads();
            s_pl[tid] += a;
            s_uh[tid] += b;
            __syncthreads();
        }
        if (i < n) {
            if (o.payload_starts) o.payload_starts[first + i] = base_pl + us.tile_pl[t] + s_pl[tid] - v.x;
            if (o.user_headers_starts) o.user_headers_starts[first + i] = base_uh + us.tile_uh[t] + s_uh[tid] - v.y;
        }
        __syncthreads();
    }
    if (blockIdx.x == 0 && tid == 0) {  // the end entry, shared with the next chained record
        if (o.payload_starts) o.payload_starts[first + n] = base_pl + us.ctl[kUpTotPl];
        if (o.user_headers_starts) o.user_headers_starts[first + n] = base_uh + us.ctl[kUpTotUh];
    }
}

// the largest m in [lo, hi] with a[m - off] <= g (a[lo - off] <= g holds on entry)
__device__ __forceinline__ uint64_t unpack_find(const uint64_t *a, uint64_t off, uint64_t lo, uint64_t hi, uint64_t g) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (a[mid - off] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// l (1..16) bytes at p as a little-endian 128-bit value, then moved up by k bytes (k + l <= 16).
// wide: the 16 bytes at p lie inside the record, so one unaligned 16-B load serves.
__device__ __forceinline__ void unpack_segment(const uint8_t *p, uint32_t l, uint32_t k, bool wide, uint64_t &lo,
                                               uint64_t &hi) {
    uint64_t a = 0, b = 0;
    if (wide) {
        const uint4 v = ld128_any(p);
        a = (uint64_t)v.x | ((uint64_t)v.y << 32);
        b = (uint64_t)v.z | ((uint64_t)v.w << 32);
        if (l < 8) a &= (1ull << (8 * l)) - 1;
        if (l <= 8) b = 0;
        else if (l < 16) b &= (1ull << (8 * (l - 8))) - 1;
    } else {
        for (uint32_t j = 0; j < l; ++j) {
            const uint64_t v = p[j];
            if (j < 8) a |= v << (8 * j);
            else b |= v << (8 * (j - 8));
        }
    }
    if (k >= 8) {
        b = a << (8 * (k - 8));
        a = 0;
    } else if (k) {
        b = (b << (8 * k)) | (a >> (64 - 8 * k));
        a <<= 8 * k;
    }
    lo |= a;
    hi |= b;
}

// which = 0: payloads, 1: user headers. starts = the array's starts (absolute positions in
// dst, entry [first + n] = end), dst = the whole output array.
__global__ __launch_bounds__(256) void k_unpack_copy(const uint8_t *__restrict__ rec, const uint64_t *__restrict__ pos,
                                                     const uint64_t *__restrict__ starts, uint8_t *__restrict__ dst,
                                                     uint32_t which, UnpackScratch us) {
    __shared__ uint64_t s_st[kUpStage];   // the span's starts
    __shared__ uint64_t s_src[kUpStage];  // rec + s_src[m] + g = the source of array byte g of message m
    __shared__ uint64_t s_m[2];
    if (!us.ctl[kUpOk]) return;
    const uint64_t tot = us.ctl[kUpTotPl + which];
    if (!tot) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t n = us.ctl[kUpCount], base = us.ctl[kUpBasePl + which];
    const uint64_t rec_len = us.ctl[kUpRecLen];
    const uint64_t *st = starts + us.ctl[kUpFirst];
    // 16-B chunks of the destination ADDRESS space: chunk 0 holds the array's first byte
    const uint64_t lead = (uint64_t)((uintptr_t)(dst + base) & 15);
    const uint64_t nchunks = (lead + tot + 15) / 16;
    const uint64_t nspans = (nchunks + kUpChunks - 1) / kUpChunks;
    for (uint64_t sp = blockIdx.x; sp < nspans; sp += gridDim.x) {
        const uint64_t c_lo = sp * kUpChunks, c_hi = min(nchunks, c_lo + kUpChunks);
        if (tid == 0) {  // the messages under the span's first and last byte
            const uint64_t b_lo = c_lo ? c_lo * 16 - lead : 0, b_hi = min(c_hi * 16 - lead, tot);
            s_m[0] = unpack_find(st, 0, 0, n - 1, base + b_lo);
            s_m[1] = unpack_find(st, 0, s_m[0], n - 1, base + b_hi - 1);
        }
        __syncthreads();
        const uint64_t m_lo = s_m[0], m_hi = s_m[1];
        // (more than kUpStage - 2 messages under one span, under 32 B each: read in place)
        const bool staged = m_hi - m_lo + 2 <= kUpStage;
        if (staged)
            for (uint64_t k = tid; k < m_hi - m_lo + 2; k += 256) {
                const uint64_t mm = m_lo + k;
                s_st[k] = st[mm];
                if (mm <= m_hi) s_src[k] = kHdr + pos[mm] + kFrameHdr + (which ? us.lens[mm].x : 0u) - st[mm];
            }
        __syncthreads();
        const uint64_t *a = staged ? s_st : st;
        const uint64_t off = staged ? m_lo : 0;
        auto src_of = [&](uint64_t mm) -> uint64_t {
            return staged ? s_src[mm - m_lo] : kHdr + pos[mm] + kFrameHdr + (which ? us.lens[mm].x : 0u) - st[mm];
        };
        uint64_t m = m_lo;
        for (uint64_t c = c_lo + tid; c < c_hi; c += 256) {
            const uint64_t b_lo = c ? c * 16 - lead : 0, b_hi = min(c * 16 + 16 - lead, tot);
            uint64_t g = base + b_lo;
            const uint64_t g_end = base + b_hi;
            if (a[m + 1 - off] <= g) m = unpack_find(a, off, m + 1, m_hi, g);
            if (b_hi - b_lo == 16) {
                uint4 v;
                if (a[m + 1 - off] >= g_end) {  // inside one message
                    v = ld128_any(rec + src_of(m) + g);
                } else {
                    // messages meet inside this chunk: one piece per message, assembled in registers
                    uint64_t lo = 0, hi = 0, mb = m;
                    for (uint64_t q = g; q < g_end;) {
                        while (a[mb + 1 - off] <= q) ++mb;
                        const uint64_t q_end = min(a[mb + 1 - off], g_end);
                        const uint64_t so = src_of(mb) + q;
                        unpack_segment(rec + so, (uint32_t)(q_end - q), (uint32_t)(q - g), so + 16 <= rec_len, lo, hi);
                        q = q_end;
                    }
                    v = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
                }
                *(uint4 *)(dst + g) = v;
            } else {
                // the array's first or last chunk, not whole: byte-wise, only the array's own bytes
                uint64_t mb = m;
                for (; g < g_end; ++g) {
                    while (a[mb + 1 - off] <= g) ++mb;
                    dst[g] = rec[src_of(mb) + g];
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace iggy


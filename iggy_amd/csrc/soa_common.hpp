// soa_common.hpp — what the stages over an iggy_unpacked_messages share (the unpack,
// unpack.hip; the select, select.hip; the route, route.hip), each piece written once:
// the control words a stage's scan kernel publishes for the kernels after it, the 256-thread
// scan and reduction in LDS, tile sums to tile offsets, the placement of a stage's output
// behind a cursor, the scatter of the fixed-width arrays, and the byte copy k_soa_copy.
#pragma once
#include "codec_common.hpp"

namespace iggy {

constexpr uint32_t kSoaSpan = 32u << 10;       // destination bytes per copy span
constexpr uint32_t kSoaChunks = kSoaSpan / 16;  // 16-B chunks per span
constexpr uint32_t kSoaStage = 1024;           // starts of a span staged in LDS (else read in place)
// control words [8]. kSoaAux is the stage's own: the record's batch_length (unpack), the
// source messages examined (select, route).
constexpr uint32_t kSoaOk = 0, kSoaFirst = 1, kSoaCount = 2, kSoaBasePl = 3, kSoaBaseUh = 4, kSoaTotPl = 5,
                   kSoaTotUh = 6, kSoaAux = 7;

// a message's byte length: the lengths array when the source has one, else its two starts
__device__ __forceinline__ uint32_t soa_len(const uint32_t *lens, const uint64_t *starts, uint64_t i) {
    if (lens) return lens[i];
    if (starts) return (uint32_t)(starts[i + 1] - starts[i]);
    return 0;
}

// a device-resident source count the source's arrays and the stage's scratch can hold
__device__ __forceinline__ bool soa_gate(uint64_t n, const iggy_unpacked_messages &src, uint64_t max_messages) {
    return n <= src.cap_messages && n <= max_messages;
}

// Inclusive scan of [256] LDS arrays (Hillis-Steele), all of them in one loop: two barriers
// per step however many arrays. The caller has stored s[tid] and synchronised.
template <class... T>
__device__ __forceinline__ void soa_scan(uint32_t tid, T *...s) {
    for (uint32_t k = 1; k < 256; k <<= 1) {
        const auto add = [&](T... below) {  // (the arguments are loaded before the body runs)
            __syncthreads();
            ((s[tid] += below), ...);
            __syncthreads();
        };
        add((tid >= k ? s[tid - k] : T(0))...);
    }
}

// Tree reduction of [256] LDS arrays into entry [0], in one loop: sums of every s and, with
// kMinMax, the minimum of mn and the maximum of mx (else they are not read: a test of the
// pointers at run time would split every step's LDS loads in two). Ends synchronised.
template <bool kMinMax, class... T>
__device__ __forceinline__ void soa_reduce(uint32_t tid, uint32_t *mn, uint32_t *mx, T *...s) {
    for (uint32_t k = 128; k > 0; k >>= 1) {
        if (tid < k) {
            ((s[tid] += s[tid + k]), ...);
            if constexpr (kMinMax) {
                mn[tid] = min(mn[tid], mn[tid + k]);
                mx[tid] = max(mx[tid], mx[tid + k]);
            }
        }
        __syncthreads();
    }
}

template <int N>
struct SoaTotals {
    uint64_t sum[N];
    uint32_t mn, mx;
};

// One workgroup: N arrays of tile sums become tile offsets in place (exclusive scan, 256
// tiles per round with a carry); the totals come back to every thread. kMinMax: tile_mm
// holds per tile the min and max of a quantity, [2 * ntiles], folded into mn / mx.
template <bool kMinMax, int N>
__device__ __forceinline__ SoaTotals<N> soa_tile_offsets(uint32_t tid, uint64_t ntiles, uint64_t *const (&tile)[N],
                                                         const uint32_t *tile_mm) {
    static_assert(N == 2 || N == 3, "two or three sums");
    __shared__ uint64_t s[N][256];
    __shared__ uint32_t s_mn[256], s_mx[256];  // (not allocated without kMinMax: never referenced)
    __shared__ uint64_t c_sum[N];
    __shared__ uint32_t c_mn, c_mx;
    if (tid == 0) {
        for (int q = 0; q < N; ++q) c_sum[q] = 0;
        if constexpr (kMinMax) {
            c_mn = 0xFFFFFFFFu;
            c_mx = 0;
        }
    }
    __syncthreads();
    for (uint64_t t0 = 0; t0 < ntiles; t0 += 256) {
        const uint64_t t = t0 + tid;
        // (every global load before the first LDS store: the loads of a round are in flight together)
        uint64_t v[N];
        for (int q = 0; q < N; ++q) v[q] = t < ntiles ? tile[q][t] : 0;
        if constexpr (kMinMax) {
            const uint32_t mn = t < ntiles ? tile_mm[2 * t] : 0xFFFFFFFFu, mx = t < ntiles ? tile_mm[2 * t + 1] : 0;
            s_mn[tid] = mn;
            s_mx[tid] = mx;
        }
        for (int q = 0; q < N; ++q) s[q][tid] = v[q];
        __syncthreads();
        if constexpr (N == 2) soa_scan(tid, s[0], s[1]);
        else soa_scan(tid, s[0], s[1], s[2]);
        if (t < ntiles)
            for (int q = 0; q < N; ++q) tile[q][t] = c_sum[q] + s[q][tid] - v[q];
        if constexpr (kMinMax) soa_reduce<true>(tid, s_mn, s_mx);
        else __syncthreads();
        if (tid == 0) {
            for (int q = 0; q < N; ++q) c_sum[q] += s[q][255];
            if constexpr (kMinMax) {
                c_mn = min(c_mn, s_mn[0]);
                c_mx = max(c_mx, s_mx[0]);
            }
        }
        __syncthreads();
    }
    SoaTotals<N> tot{};
    for (int q = 0; q < N; ++q) tot.sum[q] = c_sum[q];
    if constexpr (kMinMax) {
        tot.mn = c_mn;
        tot.mx = c_mx;
    }
    return tot;
}

// Where a stage's `count` messages of tot_pl + tot_uh bytes land in the output arrays o: behind
// the cursor (at 0 without one), and whether the capacities of the arrays wanted hold them.
struct SoaPlacement {
    uint64_t first, base_pl, base_uh;
    uint64_t need_m, need_pl, need_uh;  // the sizes the arrays must have
    bool fits;
};

__device__ __forceinline__ SoaPlacement soa_place(const iggy_unpack_cursor *cur, const iggy_unpacked_messages &o,
                                                  uint64_t count, uint64_t tot_pl, uint64_t tot_uh) {
    SoaPlacement p;
    p.first = cur ? cur->messages : 0;
    p.base_pl = cur ? cur->payload_bytes : 0;
    p.base_uh = cur ? cur->user_headers_bytes : 0;
    p.need_m = sat_add(p.first, count);
    p.need_pl = sat_add(p.base_pl, tot_pl);
    p.need_uh = sat_add(p.base_uh, tot_uh);
    p.fits = p.need_m <= o.cap_messages && (!o.payloads || p.need_pl <= o.cap_payload_bytes) &&
             (!o.user_headers || p.need_uh <= o.cap_user_headers_bytes);
    return p;
}

__device__ __forceinline__ iggy_wire_error soa_capacity_error(const SoaPlacement &p) {
    iggy_wire_error e{};
    e.kind = IGGY_ERR_CAPACITY;
    e.a = p.need_m;
    e.b = p.need_pl;
    e.c = p.need_uh;
    return e;
}

// One thread, after the stage's result is written: the cursor's advance when the output
// fits, and the control words.
__device__ __forceinline__ void soa_publish(uint64_t *ctl, iggy_unpack_cursor *cur, const SoaPlacement &p,
                                            uint64_t count, uint64_t tot_pl, uint64_t tot_uh, uint64_t aux) {
    if (cur && p.fits) {
        cur->messages = p.need_m;
        cur->payload_bytes = p.need_pl;
        cur->user_headers_bytes = p.need_uh;
    }
    ctl[kSoaOk] = p.fits ? 1 : 0;
    ctl[kSoaFirst] = p.first;
    ctl[kSoaCount] = count;
    ctl[kSoaBasePl] = p.base_pl;
    ctl[kSoaBaseUh] = p.base_uh;
    ctl[kSoaTotPl] = tot_pl;
    ctl[kSoaTotUh] = tot_uh;
    ctl[kSoaAux] = aux;
}

// the fixed-width arrays of source message i to destination index d (pl, uh: its lengths)
__device__ __forceinline__ void soa_scatter_fixed(const iggy_unpacked_messages &src, uint64_t i,
                                                  const iggy_unpacked_messages &o, uint64_t d, uint32_t pl,
                                                  uint32_t uh) {
    if (o.ids) {
        o.ids[2 * d] = src.ids[2 * i];
        o.ids[2 * d + 1] = src.ids[2 * i + 1];
    }
    if (o.checksums) o.checksums[d] = src.checksums[i];
    if (o.offsets) o.offsets[d] = src.offsets[i];
    if (o.timestamps) o.timestamps[d] = src.timestamps[i];
    if (o.origin_timestamps) o.origin_timestamps[d] = src.origin_timestamps[i];
    if (o.payload_lengths) o.payload_lengths[d] = pl;
    if (o.user_headers_lengths) o.user_headers_lengths[d] = uh;
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
// wide: the 16 bytes at p lie inside the source, so one unaligned 16-B load serves.
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

// The sources of k_soa_copy: where output message m's bytes lie (bytes + offset(m)), and the
// exclusive bound below which a 16-B load of a boundary piece may be issued (ctl: the
// control words, st: the destination starts of the stage's n messages, entry [n] = end).

// a record's frames: which = 0 the payloads, 1 the user headers (unpack)
struct SoaRecordSource {
    const uint8_t *__restrict__ bytes;  // the record
    const uint64_t *__restrict__ pos;   // frame positions in its blob
    const uint2 *lens;                  // payload_length, user_headers_length per frame
    uint32_t which;
    __device__ __forceinline__ uint64_t offset(uint64_t m) const {
        return kHdr + pos[m] + kFrameHdr + (which ? lens[m].x : 0u);
    }
    __device__ __forceinline__ uint64_t wide_end(const uint64_t *ctl, const uint64_t *, uint64_t) const {
        return ctl[kSoaAux];  // the record's batch_length
    }
};

// message sidx[m] of a byte array with starts. kSourceOrder (the select): the messages are
// in source order, so the last one's end is the highest byte read at all. Any order (the
// route): the end of the source's used bytes.
template <bool kSourceOrder>
struct SoaIndexedSource {
    const uint8_t *__restrict__ bytes;
    const uint64_t *__restrict__ sstarts;
    const uint64_t *sidx;
    __device__ __forceinline__ uint64_t offset(uint64_t m) const { return sstarts[sidx[m]]; }
    __device__ __forceinline__ uint64_t wide_end(const uint64_t *ctl, const uint64_t *st, uint64_t n) const {
        return kSourceOrder ? sstarts[sidx[n - 1]] + (st[n] - st[n - 1]) : sstarts[ctl[kSoaAux]];
    }
};

// The byte copy of the three stages. Work split by OUTPUT bytes: a workgroup owns 32 KiB
// spans of the destination (16-B aligned to the destination address), finds the messages
// under a span by binary search in the starts, and moves one 16-B destination chunk per
// thread per step: an aligned store of an unaligned load where the chunk lies inside one
// message, assembled in registers where messages meet inside the chunk, byte-wise at the
// array's ends, so a thread only ever writes bytes of the array's own range.
// which = 0: payloads, 1: user headers. starts = the array's starts (absolute positions in
// dst, entry [first + n] = end), dst = the whole output array.
template <class Source>
__global__ __launch_bounds__(256) void k_soa_copy(Source src, const uint64_t *__restrict__ starts,
                                                  uint8_t *__restrict__ dst, uint32_t which, const uint64_t *ctl) {
    __shared__ uint64_t s_st[kSoaStage];   // the span's starts
    __shared__ uint64_t s_src[kSoaStage];  // src.bytes + s_src[m] + g = the source of array byte g of message m
    __shared__ uint64_t s_m[2];
    if (!ctl[kSoaOk]) return;
    const uint64_t tot = ctl[kSoaTotPl + which];
    if (!tot) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t n = ctl[kSoaCount], base = ctl[kSoaBasePl + which];
    const uint64_t *st = starts + ctl[kSoaFirst];
    const uint64_t src_end = src.wide_end(ctl, st, n);
    // 16-B chunks of the destination ADDRESS space: chunk 0 holds the array's first byte
    const uint64_t lead = (uint64_t)((uintptr_t)(dst + base) & 15);
    const uint64_t nchunks = (lead + tot + 15) / 16;
    const uint64_t nspans = (nchunks + kSoaChunks - 1) / kSoaChunks;
    for (uint64_t sp = blockIdx.x; sp < nspans; sp += gridDim.x) {
        const uint64_t c_lo = sp * kSoaChunks, c_hi = min(nchunks, c_lo + kSoaChunks);
        if (tid == 0) {  // the messages under the span's first and last byte
            const uint64_t b_lo = c_lo ? c_lo * 16 - lead : 0, b_hi = min(c_hi * 16 - lead, tot);
            s_m[0] = unpack_find(st, 0, 0, n - 1, base + b_lo);
            s_m[1] = unpack_find(st, 0, s_m[0], n - 1, base + b_hi - 1);
        }
        __syncthreads();
        const uint64_t m_lo = s_m[0], m_hi = s_m[1];
        // (more than kSoaStage - 2 messages under one span, under 32 B each: read in place)
        const bool staged = m_hi - m_lo + 2 <= kSoaStage;
        if (staged)
            for (uint64_t k = tid; k < m_hi - m_lo + 2; k += 256) {
                const uint64_t mm = m_lo + k;
                s_st[k] = st[mm];
                if (mm <= m_hi) s_src[k] = src.offset(mm) - st[mm];
            }
        __syncthreads();
        const uint64_t *a = staged ? s_st : st;
        const uint64_t off = staged ? m_lo : 0;
        auto src_of = [&](uint64_t mm) -> uint64_t { return staged ? s_src[mm - m_lo] : src.offset(mm) - st[mm]; };
        uint64_t m = m_lo;
        for (uint64_t c = c_lo + tid; c < c_hi; c += 256) {
            const uint64_t b_lo = c ? c * 16 - lead : 0, b_hi = min(c * 16 + 16 - lead, tot);
            uint64_t g = base + b_lo;
            const uint64_t g_end = base + b_hi;
            if (a[m + 1 - off] <= g) m = unpack_find(a, off, m + 1, m_hi, g);
            if (b_hi - b_lo == 16) {
                uint4 v;
                if (a[m + 1 - off] >= g_end) {  // inside one message
                    v = ld128_any(src.bytes + src_of(m) + g);
                } else {
                    // messages meet inside this chunk: one piece per message, assembled in registers
                    uint64_t lo = 0, hi = 0, mb = m;
                    for (uint64_t q = g; q < g_end;) {
                        while (a[mb + 1 - off] <= q) ++mb;
                        const uint64_t q_end = min(a[mb + 1 - off], g_end);
                        const uint64_t so = src_of(mb) + q;
                        unpack_segment(src.bytes + so, (uint32_t)(q_end - q), (uint32_t)(q - g), so + 16 <= src_end, lo,
                                       hi);
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
                    dst[g] = src.bytes[src_of(mb) + g];
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace iggy

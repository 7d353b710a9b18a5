// select.hip — device-side select: a conjunction of typed clauses over the per-message
// arrays of an iggy_unpacked_messages (and header columns), then the stable compaction of
// the kept messages into a second set of arrays (include/iggy_codec.h "select").
//
//  k_sel_flags  : one thread per source message, 256-message tiles: the clauses (kernel
//                 arguments, select_clause.hpp) over only the arrays they name, a keep flag,
//                 and per tile the kept count, the kept payload / user-header byte sums and
//                 the min / max kept payload length.
//  k_sel_scan   : one WG: exclusive scan of the tile sums (u64), the gate on the count, the
//                 cursor's bases, the capacity verdict, the result, the cursor's advance.
//  k_sel_fields : per tile the scan of the flags and kept lengths -> destination index and
//                 starts; the fixed-width arrays of the kept messages, the source index.
//  k_sel_copy   : the unpack's copy form (k_unpack_copy, unpack.hip) with another source
//                 address: work split by OUTPUT bytes, 32 KiB destination spans cut at 16-B
//                 destination addresses, the messages under a span found by binary search in
//                 the destination starts, one 16-B destination chunk per thread per step.
//
// Positions come from prefix sums alone (no atomics): the output is bit-identical from run
// to run. Every kernel reads the source count from device memory; the host sizes the grids
// from the capacities alone.
#include "codec_common.hpp"
#include "select_clause.hpp"

namespace iggy {

constexpr uint32_t kSelTile = 256;
// control words published by k_sel_scan for the kernels after it
constexpr uint32_t kSelOk = 0, kSelFirst = 1, kSelCount = 2, kSelBasePl = 3, kSelBaseUh = 4, kSelTotPl = 5,
                   kSelTotUh = 6, kSelExamined = 7;

struct SelScratch {
    uint64_t *ctl;          // [8] kSel* words
    uint64_t *tile_n;       // [ntiles] kept per tile -> tile offsets after the scan
    uint64_t *tile_pl;      // [ntiles]
    uint64_t *tile_uh;      // [ntiles]
    uint32_t *tile_mm;      // [2 * ntiles] min, max kept payload length
    uint64_t *sidx;         // [max_messages] source index of kept message j (0-based)
    uint8_t *flags;         // [max_messages]
    uint64_t max_messages;  // messages the scratch holds (>= the source's cap_messages)
};

// a message's byte length: the lengths array when the source has one, else its two starts
__device__ __forceinline__ uint32_t sel_len(const uint32_t *lens, const uint64_t *starts, uint64_t i) {
    if (lens) return lens[i];
    if (starts) return (uint32_t)(starts[i + 1] - starts[i]);
    return 0;
}

__device__ __forceinline__ bool sel_gate(uint64_t n, const iggy_unpacked_messages &src, const SelScratch &ss) {
    return n <= src.cap_messages && n <= ss.max_messages;
}

__global__ __launch_bounds__(256) void k_sel_flags(iggy_unpacked_messages src, const uint64_t *d_count,
                                                   SelProgram prog, SelScratch ss) {
    __shared__ uint64_t s_pl[256], s_uh[256];
    __shared__ uint32_t s_n[256], s_mn[256], s_mx[256];
    const uint64_t n = *d_count;
    if (!sel_gate(n, src, ss)) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t ntiles = (n + kSelTile - 1) / kSelTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i = t * kSelTile + tid;
        bool keep = false;
        uint32_t pl = 0, uh = 0;
        if (i < n) {
            keep = sel_keep(prog, src, i);
            ss.flags[i] = keep ? 1 : 0;
            if (keep) {
                pl = sel_len(src.payload_lengths, src.payload_starts, i);
                uh = sel_len(src.user_headers_lengths, src.user_headers_starts, i);
            }
        }
        s_n[tid] = keep ? 1 : 0;
        s_pl[tid] = pl;
        s_uh[tid] = uh;
        s_mn[tid] = keep ? pl : 0xFFFFFFFFu;
        s_mx[tid] = pl;
        __syncthreads();
        for (uint32_t k = 128; k > 0; k >>= 1) {
            if (tid < k) {
                s_n[tid] += s_n[tid + k];
                s_pl[tid] += s_pl[tid + k];
                s_uh[tid] += s_uh[tid + k];
                s_mn[tid] = min(s_mn[tid], s_mn[tid + k]);
                s_mx[tid] = max(s_mx[tid], s_mx[tid + k]);
            }
            __syncthreads();
        }
        if (tid == 0) {
            ss.tile_n[t] = s_n[0];
            ss.tile_pl[t] = s_pl[0];
            ss.tile_uh[t] = s_uh[0];
            ss.tile_mm[2 * t] = s_mn[0];
            ss.tile_mm[2 * t + 1] = s_mx[0];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_sel_scan(iggy_unpacked_messages src, const uint64_t *d_count,
                                                  iggy_unpacked_messages o, iggy_unpack_cursor *cur, SelScratch ss,
                                                  iggy_select_result *res) {
    __shared__ uint64_t s_n[256], s_pl[256], s_uh[256];
    __shared__ uint32_t s_mn[256], s_mx[256];
    __shared__ uint64_t carry_n, carry_pl, carry_uh;
    __shared__ uint32_t carry_mn, carry_mx;
    const uint32_t tid = threadIdx.x;
    const uint64_t n = *d_count;
    const uint64_t first = cur ? cur->messages : 0;
    if (!sel_gate(n, src, ss)) {
        if (tid == 0) {
            iggy_select_result r{};
            r.error.kind = IGGY_ERR_INVALID_ARGUMENT;
            r.error.a = n;
            r.examined = n;
            r.first_message = first;
            *res = r;
            ss.ctl[kSelOk] = 0;
        }
        return;
    }
    const uint64_t ntiles = (n + kSelTile - 1) / kSelTile;
    if (tid == 0) { carry_n = 0; carry_pl = 0; carry_uh = 0; carry_mn = 0xFFFFFFFFu; carry_mx = 0; }
    __syncthreads();
    for (uint64_t t0 = 0; t0 < ntiles; t0 += 256) {
        const uint64_t t = t0 + tid;
        const uint64_t vn = t < ntiles ? ss.tile_n[t] : 0;
        const uint64_t vpl = t < ntiles ? ss.tile_pl[t] : 0;
        const uint64_t vuh = t < ntiles ? ss.tile_uh[t] : 0;
        s_n[tid] = vn;
        s_pl[tid] = vpl;
        s_uh[tid] = vuh;
        s_mn[tid] = t < ntiles ? ss.tile_mm[2 * t] : 0xFFFFFFFFu;
        s_mx[tid] = t < ntiles ? ss.tile_mm[2 * t + 1] : 0;
        __syncthreads();
        for (uint32_t k = 1; k < 256; k <<= 1) {  // inclusive scan (Hillis-Steele in LDS, as k_unpack_scan)
            const uint64_t a = tid >= k ? s_n[tid - k] : 0;
            const uint64_t b = tid >= k ? s_pl[tid - k] : 0;
            const uint64_t c = tid >= k ? s_uh[tid - k] : 0;
            __syncthreads();
            s_n[tid] += a;
            s_pl[tid] += b;
            s_uh[tid] += c;
            __syncthreads();
        }
        if (t < ntiles) {
            ss.tile_n[t] = carry_n + s_n[tid] - vn;
            ss.tile_pl[t] = carry_pl + s_pl[tid] - vpl;
            ss.tile_uh[t] = carry_uh + s_uh[tid] - vuh;
        }
        for (uint32_t k = 128; k > 0; k >>= 1) {
            if (tid < k) {
                s_mn[tid] = min(s_mn[tid], s_mn[tid + k]);
                s_mx[tid] = max(s_mx[tid], s_mx[tid + k]);
            }
            __syncthreads();
        }
        if (tid == 0) {
            carry_n += s_n[255];
            carry_pl += s_pl[255];
            carry_uh += s_uh[255];
            carry_mn = min(carry_mn, s_mn[0]);
            carry_mx = max(carry_mx, s_mx[0]);
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const uint64_t base_pl = cur ? cur->payload_bytes : 0, base_uh = cur ? cur->user_headers_bytes : 0;
    const uint64_t need_m = sat_add(first, carry_n), need_pl = sat_add(base_pl, carry_pl),
                   need_uh = sat_add(base_uh, carry_uh);
    const bool fits = need_m <= o.cap_messages && (!o.payloads || need_pl <= o.cap_payload_bytes) &&
                      (!o.user_headers || need_uh <= o.cap_user_headers_bytes);
    iggy_select_result r{};
    r.examined = n;
    r.first_message = first;
    if (fits) {
        r.count = carry_n;
        r.payload_bytes = carry_pl;
        r.user_headers_bytes = carry_uh;
        r.min_payload_length = carry_n ? carry_mn : 0;
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
    ss.ctl[kSelOk] = fits ? 1 : 0;
    ss.ctl[kSelFirst] = first;
    ss.ctl[kSelCount] = carry_n;
    ss.ctl[kSelBasePl] = base_pl;
    ss.ctl[kSelBaseUh] = base_uh;
    ss.ctl[kSelTotPl] = carry_pl;
    ss.ctl[kSelTotUh] = carry_uh;
    ss.ctl[kSelExamined] = n;
}

__global__ __launch_bounds__(256) void k_sel_fields(iggy_unpacked_messages src, iggy_unpacked_messages o,
                                                    uint64_t *source_index, SelScratch ss) {
    __shared__ uint64_t s_pl[256], s_uh[256];
    __shared__ uint32_t s_n[256];
    if (!ss.ctl[kSelOk]) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t first = ss.ctl[kSelFirst], n = ss.ctl[kSelExamined], kept = ss.ctl[kSelCount];
    const uint64_t base_pl = ss.ctl[kSelBasePl], base_uh = ss.ctl[kSelBaseUh];
    const uint64_t ntiles = (n + kSelTile - 1) / kSelTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i = t * kSelTile + tid;
        const bool keep = i < n && ss.flags[i] != 0;
        uint32_t pl = 0, uh = 0;
        if (keep) {
            pl = sel_len(src.payload_lengths, src.payload_starts, i);
            uh = sel_len(src.user_headers_lengths, src.user_headers_starts, i);
        }
        s_n[tid] = keep ? 1 : 0;
        s_pl[tid] = pl;
        s_uh[tid] = uh;
        __syncthreads();
        for (uint32_t k = 1; k < 256; k <<= 1) {
            const uint32_t a = tid >= k ? s_n[tid - k] : 0;
            const uint64_t b = tid >= k ? s_pl[tid - k] : 0;
            const uint64_t c = tid >= k ? s_uh[tid - k] : 0;
            __syncthreads();
            s_n[tid] += a;
            s_pl[tid] += b;
            s_uh[tid] += c;
            __syncthreads();
        }
        if (keep) {
            const uint64_t j = ss.tile_n[t] + s_n[tid] - 1;  // < kept: the scan's verdict covers first + j
            const uint64_t d = first + j;
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
            if (o.payload_starts) o.payload_starts[d] = base_pl + ss.tile_pl[t] + s_pl[tid] - pl;
            if (o.user_headers_starts) o.user_headers_starts[d] = base_uh + ss.tile_uh[t] + s_uh[tid] - uh;
            ss.sidx[j] = i;
            if (source_index) source_index[d] = i;
        }
        __syncthreads();
    }
    if (blockIdx.x == 0 && tid == 0) {  // the end entry, shared with the next chained select / unpack
        if (o.payload_starts) o.payload_starts[first + kept] = base_pl + ss.ctl[kSelTotPl];
        if (o.user_headers_starts) o.user_headers_starts[first + kept] = base_uh + ss.ctl[kSelTotUh];
    }
}

// which = 0: payloads, 1: user headers. sbytes / sstarts = the source array and its starts,
// starts = the destination's starts (absolute positions in dst, entry [first + kept] = end),
// dst = the whole output array. Source of destination byte g of kept message m:
// sbytes + sstarts[sidx[m]] + (g - starts[first + m]).
// kSourceOrder: the kept messages are in source order (the select). false (the route,
// route.hip): any order, the wide loads are bounded by the source's used bytes instead.
template <bool kSourceOrder = true>
__global__ __launch_bounds__(256) void k_sel_copy(const uint8_t *__restrict__ sbytes,
                                                  const uint64_t *__restrict__ sstarts,
                                                  const uint64_t *__restrict__ starts, uint8_t *__restrict__ dst,
                                                  uint32_t which, SelScratch ss) {
    __shared__ uint64_t s_st[kUpStage];   // the span's destination starts
    __shared__ uint64_t s_src[kUpStage];  // sbytes + s_src[m] + g = the source of array byte g of message m
    __shared__ uint64_t s_m[2];
    if (!ss.ctl[kSelOk]) return;
    const uint64_t tot = ss.ctl[kSelTotPl + which];
    if (!tot) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t n = ss.ctl[kSelCount], base = ss.ctl[kSelBasePl + which];
    const uint64_t *st = starts + ss.ctl[kSelFirst];
    // wide (16-B) loads of a boundary piece stay below the end of the last kept message's
    // source bytes (kept messages are in source order: it is the highest byte read at all)
    const uint64_t src_end =
        kSourceOrder ? sstarts[ss.sidx[n - 1]] + (st[n] - st[n - 1]) : sstarts[ss.ctl[kSelExamined]];
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
                if (mm <= m_hi) s_src[k] = sstarts[ss.sidx[mm]] - st[mm];
            }
        __syncthreads();
        const uint64_t *a = staged ? s_st : st;
        const uint64_t off = staged ? m_lo : 0;
        auto src_of = [&](uint64_t mm) -> uint64_t {
            return staged ? s_src[mm - m_lo] : sstarts[ss.sidx[mm]] - st[mm];
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
                    v = ld128_any(sbytes + src_of(m) + g);
                } else {
                    // messages meet inside this chunk: one piece per message, assembled in registers
                    uint64_t lo = 0, hi = 0, mb = m;
                    for (uint64_t q = g; q < g_end;) {
                        while (a[mb + 1 - off] <= q) ++mb;
                        const uint64_t q_end = min(a[mb + 1 - off], g_end);
                        const uint64_t so = src_of(mb) + q;
                        unpack_segment(sbytes + so, (uint32_t)(q_end - q), (uint32_t)(q - g), so + 16 <= src_end, lo, hi);
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
                    dst[g] = sbytes[src_of(mb) + g];
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace iggy

// route.hip — device-side route: the partition of every message of an
// iggy_unpacked_messages by the reference's rule, XXH32(key) % partitions (route_key.hpp,
// xxh32.hpp), then the stable N-way split of the routed messages into a second set of
// arrays ordered by (partition, source index) (include/iggy_codec.h "route"). One 8-bit
// radix-sort pass that carries the messages.
//
//  k_route_keys   : 2048-message tiles, one thread per message in 8 rounds: the gate, the
//                   mask, the key at its (arbitrary) address, the XXH32; the partition into
//                   scratch (u16, 0xFFFF = dropped), and per tile the partition counts (an
//                   LDS histogram, integer adds) as row t of a [tile][partition] table, plus
//                   the routed payload / user-header byte sums.
//  k_route_scan   : one WG, thread p owns partition p: its total over the tiles (the loads
//                   are coalesced across the partitions), the exclusive scan over the
//                   partitions -> d_partition_first, the capacity verdict, the result, the
//                   control words; then the table in place into destination bases (partition-
//                   major, tile-minor order).
//  k_route_fields : per tile and round the stable rank of each routed message among the
//                   round's messages of its partition: per-wave match masks from 8 ballots
//                   over the partition's bits, per-wave-per-partition counts in LDS. The
//                   destination index = the running base of the partition + the counts of the
//                   waves before + the rank. Scatters the fixed-width arrays, both lengths
//                   (to scratch, in destination order) and the source index; adds the lengths
//                   into the byte sums of 1024-message destination tiles (integer atomics
//                   whose result is not read: the sums do not depend on the order).
//  k_route_dscan  : one WG: exclusive scan of the destination tile sums.
//  k_route_starts : per destination tile the exclusive scan of the lengths + the tile offset
//                   -> payload_starts / user_headers_starts (the output has no gaps), and the
//                   two byte tables, starts[first[p]], by a search of each index in
//                   d_partition_first staged in LDS.
//  k_soa_copy<SoaIndexedSource<false>> (soa_common.hpp): the byte copy the unpack and the
//                   select share, with the wide loads bounded by the end of the source's
//                   used bytes: the destination order is not the source order here.
//
// The scans, the capacity verdict, the control words and the scatter of the fixed-width
// arrays are soa_common.hpp's. No position comes from an atomic's return value: the output
// is bit-identical from run to run. Every kernel reads the source count from device memory; the host sizes the grids
// from the capacities alone.
#include "soa_common.hpp"
#include "route_key.hpp"

namespace iggy {

constexpr uint32_t kRtRounds = 8;
constexpr uint32_t kRtTile = 256 * kRtRounds;  // source messages per tile
constexpr uint32_t kRtPer = 4;
constexpr uint32_t kRtDTile = 256 * kRtPer;    // destination messages per starts tile
constexpr uint32_t kRtParts = IGGY_ROUTE_MAX_PARTITIONS;
constexpr uint32_t kRtDrop = 0xFFFFu;          // a dropped message in RouteScratch::part

struct RouteScratch {
    uint64_t *ctl;          // [8] kSoa* words (first and the bases 0), kSoaAux = the messages examined
    uint64_t *tile_pl;      // [ntiles] routed payload bytes per source tile
    uint64_t *tile_uh;      // [ntiles]
    uint64_t *dtile_pl;     // [ndtiles] payload bytes per destination tile -> tile offsets after k_route_dscan
    uint64_t *dtile_uh;     // [ndtiles]
    uint32_t *hist;         // [ntiles][partitions] counts -> destination bases after k_route_scan
    uint64_t *sidx;         // [max_messages] source index of routed message j
    uint2 *dlens;           // [max_messages] payload_length, user_headers_length of routed message j
    uint16_t *part;         // [max_messages] partition of source message i, kRtDrop = dropped
    uint64_t max_messages;  // messages the scratch holds (>= the source's cap_messages)
};

__global__ __launch_bounds__(256) void k_route_keys(iggy_unpacked_messages src, const uint64_t *d_count,
                                                    RouteProgram prog, RouteScratch rs) {
    __shared__ uint32_t s_hist[kRtParts];
    __shared__ uint64_t s_pl[256], s_uh[256];
    const uint64_t n = *d_count;
    if (!soa_gate(n, src, rs.max_messages)) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t ntiles = (n + kRtTile - 1) / kRtTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        s_hist[tid] = 0;
        __syncthreads();
        uint64_t pl = 0, uh = 0;
        for (uint32_t r = 0; r < kRtRounds; ++r) {
            const uint64_t i = t * kRtTile + r * 256 + tid;
            if (i < n) {
                const uint32_t p = route_partition(prog, src, i);  // < partitions, or IGGY_ROUTE_DROP
                rs.part[i] = (uint16_t)(p == IGGY_ROUTE_DROP ? kRtDrop : p);
                if (p != IGGY_ROUTE_DROP) {
                    atomicAdd(&s_hist[p], 1u);
                    pl += soa_len(src.payload_lengths, src.payload_starts, i);
                    uh += soa_len(src.user_headers_lengths, src.user_headers_starts, i);
                }
            }
        }
        s_pl[tid] = pl;
        s_uh[tid] = uh;
        __syncthreads();
        soa_reduce<false>(tid, nullptr, nullptr, s_pl, s_uh);
        if (tid < prog.partitions) rs.hist[t * prog.partitions + tid] = s_hist[tid];
        if (tid == 0) {
            rs.tile_pl[t] = s_pl[0];
            rs.tile_uh[t] = s_uh[0];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_route_scan(iggy_unpacked_messages src, const uint64_t *d_count,
                                                    uint32_t partitions, iggy_unpacked_messages o, uint32_t has_out,
                                                    uint64_t *pfirst, RouteScratch rs, iggy_route_result *res) {
    __shared__ uint64_t s_a[256], s_b[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t n = *d_count;
    if (!soa_gate(n, src, rs.max_messages)) {
        if (tid == 0) {
            iggy_route_result r{};
            r.error.kind = IGGY_ERR_INVALID_ARGUMENT;
            r.error.a = n;
            r.examined = n;
            r.partitions = partitions;
            *res = r;
            rs.ctl[kSoaOk] = 0;
        }
        return;
    }
    const uint64_t ntiles = (n + kRtTile - 1) / kRtTile;
    uint64_t mine = 0;  // partition tid's messages
    if (tid < partitions)
        for (uint64_t t = 0; t < ntiles; ++t) mine += rs.hist[t * partitions + tid];
    uint64_t pl = 0, uh = 0;
    for (uint64_t t = tid; t < ntiles; t += 256) {
        pl += rs.tile_pl[t];
        uh += rs.tile_uh[t];
    }
    s_a[tid] = pl;
    s_b[tid] = uh;
    __syncthreads();
    soa_reduce<false>(tid, nullptr, nullptr, s_a, s_b);
    const uint64_t tot_pl = s_a[0], tot_uh = s_b[0];
    __syncthreads();
    s_a[tid] = mine;
    __syncthreads();
    soa_scan(tid, s_a);  // over the partitions
    const uint64_t first = s_a[tid] - mine, count = s_a[255];
    // (no cursor: the output starts at 0; without an output there is nothing to fit)
    SoaPlacement p = soa_place(nullptr, o, count, tot_pl, tot_uh);
    p.fits = p.fits || !has_out;
    if (p.fits) {
        if (tid < partitions) {
            pfirst[tid] = first;
            uint64_t run = first;  // (below 2^32: the host refuses a larger source capacity)
            for (uint64_t t = 0; t < ntiles; ++t) {
                const uint32_t v = rs.hist[t * partitions + tid];
                rs.hist[t * partitions + tid] = (uint32_t)run;
                run += v;
            }
        }
        if (tid == 0) pfirst[partitions] = count;
        const uint64_t ndt = (count + kRtDTile - 1) / kRtDTile;
        for (uint64_t t = tid; t < ndt; t += 256) {
            rs.dtile_pl[t] = 0;
            rs.dtile_uh[t] = 0;
        }
    }
    if (tid != 0) return;
    iggy_route_result r{};
    r.examined = n;
    r.partitions = partitions;
    if (p.fits) {
        r.count = count;
        r.dropped = n - count;
        r.payload_bytes = tot_pl;
        r.user_headers_bytes = tot_uh;
    } else {
        r.error = soa_capacity_error(p);
    }
    *res = r;
    soa_publish(rs.ctl, nullptr, p, count, tot_pl, tot_uh, n);
}

__global__ __launch_bounds__(256) void k_route_fields(iggy_unpacked_messages src, iggy_unpacked_messages o,
                                                      uint32_t has_out, uint32_t partitions, uint32_t *partition_of,
                                                      uint64_t *source_index, RouteScratch rs) {
    __shared__ uint32_t s_run[kRtParts];     // the next destination index of partition p
    __shared__ uint32_t s_cnt[4][kRtParts];  // this round's messages per wave and partition
    if (!rs.ctl[kSoaOk]) return;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t n = rs.ctl[kSoaAux];
    const uint64_t ntiles = (n + kRtTile - 1) / kRtTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        if (has_out && tid < partitions) s_run[tid] = rs.hist[t * partitions + tid];
        for (uint32_t r = 0; r < kRtRounds; ++r) {
            const uint64_t i = t * kRtTile + r * 256 + tid;
            const uint32_t p = i < n ? rs.part[i] : kRtDrop;
            if (partition_of && i < n) partition_of[i] = p == kRtDrop ? IGGY_ROUTE_DROP : p;
            if (!has_out) continue;
            for (uint32_t w = 0; w < 4; ++w) s_cnt[w][tid] = 0;
            __syncthreads();
            const bool live = p != kRtDrop;
            // the live lanes of this wave with the same partition (a dropped lane's mask is not used)
            uint64_t m = __ballot(live);
            for (uint32_t b = 0; b < 8; ++b) {
                const bool bit = (p >> b) & 1;
                const uint64_t v = __ballot(bit);
                m &= bit ? v : ~v;
            }
            const uint32_t rank = __popcll(m & ((1ull << lane) - 1));
            if (live && rank == 0) s_cnt[wave][p] = __popcll(m);
            __syncthreads();
            if (live) {
                uint64_t d = (uint64_t)s_run[p] + rank;  // < count: the scan's verdict covers it
                for (uint32_t w = 0; w < wave; ++w) d += s_cnt[w][p];
                const uint32_t pl = soa_len(src.payload_lengths, src.payload_starts, i);
                const uint32_t uh = soa_len(src.user_headers_lengths, src.user_headers_starts, i);
                soa_scatter_fixed(src, i, o, d, pl, uh);
                rs.dlens[d] = make_uint2(pl, uh);
                rs.sidx[d] = i;
                if (source_index) source_index[d] = i;
                // (integer sums, the results not read: their values do not depend on the order)
                if (pl) atomicAdd((unsigned long long *)&rs.dtile_pl[d / kRtDTile], (unsigned long long)pl);
                if (uh) atomicAdd((unsigned long long *)&rs.dtile_uh[d / kRtDTile], (unsigned long long)uh);
            }
            __syncthreads();
            if (tid < partitions) s_run[tid] += s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_route_dscan(RouteScratch rs) {
    if (!rs.ctl[kSoaOk]) return;
    uint64_t *const tiles[2] = {rs.dtile_pl, rs.dtile_uh};
    soa_tile_offsets<false>(threadIdx.x, (rs.ctl[kSoaCount] + kRtDTile - 1) / kRtDTile, tiles, nullptr);
}

__global__ __launch_bounds__(256) void k_route_starts(iggy_unpacked_messages o, uint32_t partitions,
                                                      const uint64_t *pfirst, uint64_t *ppl_first,
                                                      uint64_t *puh_first, RouteScratch rs) {
    __shared__ uint64_t s_pl[256], s_uh[256];
    __shared__ uint64_t s_first[kRtParts + 1];
    if (!rs.ctl[kSoaOk]) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t count = rs.ctl[kSoaCount];
    const uint64_t ndt = (count + kRtDTile - 1) / kRtDTile;
    const bool tables = ppl_first || puh_first;
    if (tables)
        for (uint32_t p = tid; p <= partitions; p += 256) s_first[p] = pfirst[p];
    __syncthreads();
    for (uint64_t t = blockIdx.x; t < ndt; t += gridDim.x) {
        const uint64_t j0 = t * kRtDTile + (uint64_t)tid * kRtPer;
        uint2 v[kRtPer];
        uint64_t a = 0, b = 0;
        for (uint32_t k = 0; k < kRtPer; ++k) {
            v[k] = j0 + k < count ? rs.dlens[j0 + k] : make_uint2(0, 0);
            a += v[k].x;
            b += v[k].y;
        }
        s_pl[tid] = a;
        s_uh[tid] = b;
        __syncthreads();
        soa_scan(tid, s_pl, s_uh);
        uint64_t sp = rs.dtile_pl[t] + s_pl[tid] - a, su = rs.dtile_uh[t] + s_uh[tid] - b;
        for (uint32_t k = 0; k < kRtPer; ++k) {
            const uint64_t j = j0 + k;
            if (j < count) {
                if (o.payload_starts) o.payload_starts[j] = sp;
                if (o.user_headers_starts) o.user_headers_starts[j] = su;
                if (tables) {  // every partition whose first message is j
                    uint32_t lo = 0, hi = partitions;
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) / 2;
                        if (s_first[mid] < j) lo = mid + 1;
                        else hi = mid;
                    }
                    for (; lo < partitions && s_first[lo] == j; ++lo) {
                        if (ppl_first) ppl_first[lo] = sp;
                        if (puh_first) puh_first[lo] = su;
                    }
                }
            }
            sp += v[k].x;
            su += v[k].y;
        }
        __syncthreads();
    }
    if (blockIdx.x == 0) {  // the end entries, and the partitions that start there (empty ones at the end)
        const uint64_t tot_pl = rs.ctl[kSoaTotPl], tot_uh = rs.ctl[kSoaTotUh];
        if (tid == 0) {
            if (o.payload_starts) o.payload_starts[count] = tot_pl;
            if (o.user_headers_starts) o.user_headers_starts[count] = tot_uh;
        }
        if (tables)
            for (uint32_t p = tid; p <= partitions; p += 256)
                if (s_first[p] == count) {
                    if (ppl_first) ppl_first[p] = tot_pl;
                    if (puh_first) puh_first[p] = tot_uh;
                }
    }
}

}  // namespace iggy

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
//  k_soa_copy<SoaIndexedSource<true>> (soa_common.hpp): the byte copy the unpack and the
//                 route share, reading kept message m at src_starts[source_index[m]].
//
// The scans, the placement behind the cursor and the control words are soa_common.hpp's.
// Positions come from prefix sums alone (no atomics): the output is bit-identical from run
// to run. Every kernel reads the source count from device memory; the host sizes the grids
// from the capacities alone.
#include "soa_common.hpp"
#include "select_clause.hpp"

namespace iggy {

constexpr uint32_t kSelTile = 256;

struct SelScratch {
    uint64_t *ctl;          // [8] kSoa* words, kSoaAux = the source messages examined
    uint64_t *tile_n;       // [ntiles] kept per tile -> tile offsets after the scan
    uint64_t *tile_pl;      // [ntiles]
    uint64_t *tile_uh;      // [ntiles]
    uint32_t *tile_mm;      // [2 * ntiles] min, max kept payload length
    uint64_t *sidx;         // [max_messages] source index of kept message j (0-based)
    uint8_t *flags;         // [max_messages]
    uint64_t max_messages;  // messages the scratch holds (>= the source's cap_messages)
};

__global__ __launch_bounds__(256) void k_sel_flags(iggy_unpacked_messages src, const uint64_t *d_count,
                                                   SelProgram prog, SelScratch ss) {
    __shared__ uint64_t s_pl[256], s_uh[256];
    __shared__ uint32_t s_n[256], s_mn[256], s_mx[256];
    const uint64_t n = *d_count;
    if (!soa_gate(n, src, ss.max_messages)) return;
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
                pl = soa_len(src.payload_lengths, src.payload_starts, i);
                uh = soa_len(src.user_headers_lengths, src.user_headers_starts, i);
            }
        }
        s_n[tid] = keep ? 1 : 0;
        s_pl[tid] = pl;
        s_uh[tid] = uh;
        s_mn[tid] = keep ? pl : 0xFFFFFFFFu;
        s_mx[tid] = pl;
        __syncthreads();
        soa_reduce<true>(tid, s_mn, s_mx, s_n, s_pl, s_uh);
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
    const uint32_t tid = threadIdx.x;
    const uint64_t n = *d_count;
    if (!soa_gate(n, src, ss.max_messages)) {
        if (tid == 0) {
            iggy_select_result r{};
            r.error.kind = IGGY_ERR_INVALID_ARGUMENT;
            r.error.a = n;
            r.examined = n;
            r.first_message = cur ? cur->messages : 0;
            *res = r;
            ss.ctl[kSoaOk] = 0;
        }
        return;
    }
    uint64_t *const tiles[3] = {ss.tile_n, ss.tile_pl, ss.tile_uh};
    const SoaTotals<3> tot = soa_tile_offsets<true>(tid, (n + kSelTile - 1) / kSelTile, tiles, ss.tile_mm);
    if (tid != 0) return;
    const uint64_t kept = tot.sum[0];
    const SoaPlacement p = soa_place(cur, o, kept, tot.sum[1], tot.sum[2]);
    iggy_select_result r{};
    r.examined = n;
    r.first_message = p.first;
    if (p.fits) {
        r.count = kept;
        r.payload_bytes = tot.sum[1];
        r.user_headers_bytes = tot.sum[2];
        r.min_payload_length = kept ? tot.mn : 0;
        r.max_payload_length = tot.mx;
    } else {
        r.error = soa_capacity_error(p);
    }
    *res = r;
    soa_publish(ss.ctl, cur, p, kept, tot.sum[1], tot.sum[2], n);
}

__global__ __launch_bounds__(256) void k_sel_fields(iggy_unpacked_messages src, iggy_unpacked_messages o,
                                                    uint64_t *source_index, SelScratch ss) {
    __shared__ uint64_t s_pl[256], s_uh[256];
    __shared__ uint32_t s_n[256];
    if (!ss.ctl[kSoaOk]) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t first = ss.ctl[kSoaFirst], n = ss.ctl[kSoaAux], kept = ss.ctl[kSoaCount];
    const uint64_t base_pl = ss.ctl[kSoaBasePl], base_uh = ss.ctl[kSoaBaseUh];
    const uint64_t ntiles = (n + kSelTile - 1) / kSelTile;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t i = t * kSelTile + tid;
        const bool keep = i < n && ss.flags[i] != 0;
        uint32_t pl = 0, uh = 0;
        if (keep) {
            pl = soa_len(src.payload_lengths, src.payload_starts, i);
            uh = soa_len(src.user_headers_lengths, src.user_headers_starts, i);
        }
        s_n[tid] = keep ? 1 : 0;
        s_pl[tid] = pl;
        s_uh[tid] = uh;
        __syncthreads();
        soa_scan(tid, s_n, s_pl, s_uh);
        if (keep) {
            const uint64_t j = ss.tile_n[t] + s_n[tid] - 1;  // < kept: the scan's verdict covers first + j
            const uint64_t d = first + j;
            soa_scatter_fixed(src, i, o, d, pl, uh);
            if (o.payload_starts) o.payload_starts[d] = base_pl + ss.tile_pl[t] + s_pl[tid] - pl;
            if (o.user_headers_starts) o.user_headers_starts[d] = base_uh + ss.tile_uh[t] + s_uh[tid] - uh;
            ss.sidx[j] = i;
            if (source_index) source_index[d] = i;
        }
        __syncthreads();
    }
    if (blockIdx.x == 0 && tid == 0) {  // the end entry, shared with the next chained select / unpack
        if (o.payload_starts) o.payload_starts[first + kept] = base_pl + ss.ctl[kSoaTotPl];
        if (o.user_headers_starts) o.user_headers_starts[first + kept] = base_uh + ss.ctl[kSoaTotUh];
    }
}

}  // namespace iggy

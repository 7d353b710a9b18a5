// user_headers.hip -- user-header validation and typed key columns on the device: the
// consumer's user_headers_map / get_user_header (common/src/types/message/
// iggy_message.rs:238-297) for every message of a device-resident record, or of the
// arrays the unpack wrote. The verdict per message is user_headers_walk.hpp's.
//
//  k_uh_init    : one thread: the gate (the unpack's) or the arrays form's count, the
//                 capacity verdict, the whole result, the control words.
//  k_uh_columns : 256-message tiles handed out by an atomic tile counter. Per tile: one
//                 thread per message finds its headers' address and length; the headers
//                 of the tile are packed, as the aligned 16-B chunks that hold them, into
//                 a 32 KiB LDS stage by coalesced 16-B loads (a chunk's message by binary
//                 search in the tile's chunk offsets), in as many rounds as the stage needs
//                 (one, unless the tile's headers pass 32 KiB); each thread walks its own
//                 TLV chain in LDS, matches the request keys (kernel arguments, so scalar
//                 data) and stores its row of every column, coalesced across the tile.
//                 A message above kUhStageMax bytes is left out of the stage and walked
//                 afterwards by a whole wave through a 4 KiB LDS window refilled with
//                 coalesced 16-B loads; the tile's other messages are stored by then,
//                 and the other workgroups go on taking tiles.
//
// The aligned 16-B chunk around a header byte lies inside that byte's page, so the
// chunk loads never touch a page the headers do not (up to 15 bytes of the neighbours
// are read, never used).
#include "codec_common.hpp"
#include "user_headers_walk.hpp"

namespace iggy {

constexpr uint32_t kUhTile = 256;                   // messages per tile (one per thread)
constexpr uint32_t kUhStageBytes = 32u << 10;       // LDS stage of a tile round
constexpr uint32_t kUhChunks = kUhStageBytes / 16;  // 16-B chunks in it
constexpr uint32_t kUhStageMax = 4096;              // headers above this are walked by a wave, in place
constexpr uint32_t kUhWin = 4096;                   // that wave's LDS window (4 windows overlay the stage)
constexpr uint32_t kUhNone = 0xFFFFFFFFu;
constexpr uint32_t kUhCtlOk = 0, kUhCtlCount = 1, kUhCtlTile = 2;  // control words (u64)
static_assert(kUhStageMax + 30 <= kUhStageBytes, "a staged message fits the stage alone");
static_assert(4 * kUhWin <= kUhStageBytes && 2 * (5 + kUhMaxField) + 16 <= kUhWin, "a pair fits a window");

// the request keys, by value with the launch (scalar loads; calls cannot overwrite each other's)
struct UhKeys {
    uint32_t nkeys;
    uint8_t kind[IGGY_HEADER_MAX_KEYS], len[IGGY_HEADER_MAX_KEYS];
    uint16_t off[IGGY_HEADER_MAX_KEYS];
    uint8_t bytes[IGGY_HEADER_MAX_KEY_BYTES];
};
struct UhOut {
    uint64_t cap;
    iggy_header_column col[IGGY_HEADER_MAX_KEYS];
    iggy_header_status *status;
    uint32_t *pairs;
};
// where the messages are: the record form (rec != nullptr) or the arrays form
struct UhSrc {
    const uint8_t *rec;
    const uint64_t *pos;
    const iggy_decode_result *dec;
    uint64_t len;
    const uint8_t *blob;
    const uint64_t *starts;
    const uint64_t *count;
};

__global__ void k_uh_init(UhSrc in, uint64_t cap, uint64_t max_frames, iggy_header_columns_result *res, uint64_t *ctl) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    iggy_header_columns_result r{};
    r.first_invalid = ~0ull;
    uint64_t n = 0;
    bool ok = true;
    if (in.rec) {
        const uint32_t gate = unpack_gate(in.dec, in.len, max_frames);
        if (gate != IGGY_OK) {
            if (in.dec->error.kind != IGGY_OK) r.error = in.dec->error;
            else r.error.kind = IGGY_ERR_INVALID_ARGUMENT;
            ok = false;
        } else {
            n = in.dec->frame_count;
        }
    } else {
        n = *in.count;
    }
    if (ok && n > cap) {
        r.error.kind = IGGY_ERR_CAPACITY;
        r.error.a = n;
        ok = false;
    }
    r.count = ok ? n : 0;
    *res = r;
    ctl[kUhCtlOk] = ok ? 1 : 0;
    ctl[kUhCtlCount] = r.count;
    ctl[kUhCtlTile] = 0;
}

struct UhStageReader {  // a message staged in LDS
    const uint8_t *s;
    __device__ __forceinline__ uint32_t b(uint32_t p) const { return s[p]; }
    __device__ __forceinline__ void ensure(uint32_t, uint32_t) const {}
};

// A long message behind a wave's LDS window. Every lane of the wave holds the same state
// and takes the same path; a refill is one coalesced sweep of aligned 16-B loads.
struct UhWindowReader {
    const uint8_t *g0;  // the 16-B aligned address at or below the message's first byte
    uint32_t lead;      // the first byte's place in that chunk
    uint32_t len;
    uint8_t *win;
    uint64_t c0 = 0, c1 = 0;  // resident chunks [c0, c1) (chunk 0 at g0)
    __device__ __forceinline__ uint32_t b(uint32_t p) const { return win[(uint64_t)lead + p - 16 * c0]; }
    __device__ __forceinline__ void ensure(uint32_t pos, uint32_t n) {
        const uint64_t lo = (uint64_t)lead + pos;
        const uint64_t hi = (uint64_t)lead + min((uint64_t)pos + n, (uint64_t)len);
        if (lo >= 16 * c0 && hi <= 16 * c1) return;
        const uint64_t total = ((uint64_t)lead + len + 15) / 16;
        const uint64_t a = lo / 16, e = min(total, a + kUhWin / 16);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the window's readers are done
        __builtin_amdgcn_wave_barrier();
        for (uint64_t c = a + (threadIdx.x & 63); c < e; c += 64)
            *(uint4 *)(win + 16 * (c - a)) = *(const uint4 *)(g0 + 16 * c);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        c0 = a;
        c1 = e;
    }
};

// kind and length first, bytes only on a match (mb(j) = byte j of the message's key)
template <class R>
__device__ __forceinline__ void uh_match(const UhKeys &keys, R &r, uint32_t *hit, uint32_t key_kind, uint32_t key_pos,
                                         uint32_t key_len, uint32_t value_kind_pos) {
    for (uint32_t k = 0; k < keys.nkeys; ++k) {
        if (keys.kind[k] != key_kind || keys.len[k] != key_len) continue;
        const uint8_t *kb = keys.bytes + keys.off[k];
        uint32_t j = 0;
        while (j < key_len && r.b(key_pos + j) == kb[j]) ++j;
        if (j == key_len) hit[k * kUhTile] = value_kind_pos;  // insert: the last pair wins
    }
}

// message i's row of every wanted array; present bits of the keys returned
template <class R>
__device__ __forceinline__ uint32_t uh_store(const UhKeys &keys, const UhOut &o, uint64_t i, const UhVerdict &v, R &r,
                                             const uint32_t *hit, bool writer) {
    if (writer) {
        if (o.status) {
            // (16 B per message, any alignment the caller chose for the array)
            st128_any((uint8_t *)(o.status + i), make_uint4(v.kind, v.reason, v.offset, v.detail));
        }
        if (o.pairs) o.pairs[i] = v.pairs;
    }
    uint32_t present = 0;
    for (uint32_t k = 0; k < keys.nkeys; ++k) {
        const uint32_t h = v.kind == IGGY_OK ? hit[k * kUhTile] : kUhNone;
        uint32_t vk = 0, vl = 0, vp = 0;
        uint32_t w[4] = {0, 0, 0, 0};
        if (h != kUhNone) {
            r.ensure(h, 5 + 16);
            vk = r.b(h);
            vl = r.b(h + 1);  // 1..255: the low byte is the length
            vp = h + 5;
            const uint32_t m = min(vl, 16u);
            for (uint32_t j = 0; j < m; ++j) w[j >> 2] |= r.b(vp + j) << (8 * (j & 3));
            present |= 1u << k;
        }
        if (!writer) continue;
        const iggy_header_column &c = o.col[k];
        if (c.value_kinds) c.value_kinds[i] = (uint8_t)vk;      // byte stores: no neighbour's byte is touched
        if (c.value_lengths) c.value_lengths[i] = (uint8_t)vl;
        if (c.value_pos) c.value_pos[i] = vp;
        if (c.values16) st128_any(c.values16 + 16 * i, make_uint4(w[0], w[1], w[2], w[3]));
    }
    return present;
}

__global__ __launch_bounds__(256) void k_uh_columns(UhSrc in, UhKeys keys, UhOut o, iggy_header_columns_result *res,
                                                    uint64_t *ctl) {
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[kUhStageBytes];
    __shared__ uint32_t s_hit[IGGY_HEADER_MAX_KEYS * kUhTile];  // [key][message]: value-kind position, or none
    __shared__ uint32_t s_off[kUhTile + 1];                     // exclusive scan of the chunk counts
    __shared__ uint64_t s_g0[kUhTile];                          // each message's first chunk address
    __shared__ uint32_t s_scan[kUhTile];
    __shared__ uint32_t s_hi;
    __shared__ uint64_t s_tile;
    if (!ctl[kUhCtlOk]) return;
    const uint64_t n = ctl[kUhCtlCount];
    const uint64_t ntiles = (n + kUhTile - 1) / kUhTile;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // this wave's counters, published once at the end (lane 0 holds them)
    uint64_t c_with = 0, c_invalid = 0, c_first = ~0ull;
    uint64_t c_found[IGGY_HEADER_MAX_KEYS];
#pragma unroll
    for (uint32_t k = 0; k < IGGY_HEADER_MAX_KEYS; ++k) c_found[k] = 0;
    auto tally = [&](uint64_t i, bool valid, bool nonempty, bool bad, uint32_t present) {
        c_with += __popcll(__ballot(valid && nonempty));
        const uint64_t badm = __ballot(valid && bad);
        if (badm) {
            c_invalid += __popcll(badm);
            // (message indices rise with the lane)
            const uint64_t f = (uint64_t)__shfl((unsigned long long)i, __ffsll((long long)badm) - 1);
            if (f < c_first) c_first = f;
        }
#pragma unroll
        for (uint32_t k = 0; k < IGGY_HEADER_MAX_KEYS; ++k)
            if (k < keys.nkeys) c_found[k] += __popcll(__ballot(valid && ((present >> k) & 1u)));
    };

    for (;;) {
        __syncthreads();  // the tile before is done with the shared arrays
        if (tid == 0) s_tile = atomicAdd((unsigned long long *)&ctl[kUhCtlTile], 1ull);
        __syncthreads();
        const uint64_t t = s_tile;
        if (t >= ntiles) break;
        const uint64_t i = t * kUhTile + tid;
        const bool valid = i < n;
        const uint8_t *src = nullptr;
        uint32_t uh = 0;
        if (valid) {
            if (in.rec) {
                const uint8_t *f = in.rec + kHdr + in.pos[i];
                const uint64_t l = ld64_any(f + 32);  // user_headers_length | payload_length << 32
                uh = (uint32_t)l;
                src = f + kFrameHdr + (l >> 32);
            } else {
                const uint64_t a = in.starts[i], b = in.starts[i + 1];
                uh = b > a ? (uint32_t)(b - a) : 0u;
                src = in.blob + a;
            }
        }
        const uint32_t lead = (uint32_t)((uintptr_t)src & 15);
        const bool staged = uh > 0 && uh <= kUhStageMax, isl = uh > kUhStageMax;
        const uint32_t nch = staged ? (lead + uh + 15) / 16 : 0;
        for (uint32_t k = 0; k < keys.nkeys; ++k) s_hit[k * kUhTile + tid] = kUhNone;
        // exclusive scan of the chunk counts (Hillis-Steele in LDS, as k_unpack_starts)
        s_scan[tid] = nch;
        __syncthreads();
        for (uint32_t k = 1; k < kUhTile; k <<= 1) {
            const uint32_t a = tid >= k ? s_scan[tid - k] : 0;
            __syncthreads();
            s_scan[tid] += a;
            __syncthreads();
        }
        const uint32_t off = s_scan[tid] - nch;
        s_off[tid] = off;
        s_g0[tid] = (uint64_t)(uintptr_t)(src - lead);
        if (tid == kUhTile - 1) s_off[kUhTile] = off + nch;
        __syncthreads();
        const uint32_t total = s_off[kUhTile];

        // messages without headers: valid, 0 pairs, every key absent
        if (valid && uh == 0) {
            UhVerdict v{IGGY_OK, 0, 0, 0, 0};
            UhStageReader r{s_stage};
            uh_store(keys, o, i, v, r, s_hit + tid, true);  // (no hit is set: nothing is read)
        }
        uint32_t present = 0;
        bool bad = false;
        for (uint32_t base = 0; base < total;) {
            // this round: the unfinished messages that fit the stage from `base` on (a prefix of them)
            const bool mine = staged && off >= base && off + nch - base <= kUhChunks;
            if (tid == 0) s_hi = base;
            __syncthreads();
            if (mine) atomicMax(&s_hi, off + nch);
            __syncthreads();
            const uint32_t hi = s_hi;
            for (uint32_t c = base + tid; c < hi; c += kUhTile) {
                uint32_t lo_m = 0, hi_m = kUhTile - 1;  // the last message with s_off <= c
                while (lo_m < hi_m) {
                    const uint32_t mid = (lo_m + hi_m + 1) / 2;
                    if (s_off[mid] <= c) lo_m = mid;
                    else hi_m = mid - 1;
                }
                const uint4 x = *(const uint4 *)(uintptr_t)(s_g0[lo_m] + 16ull * (c - s_off[lo_m]));
                *(uint4 *)(s_stage + 16 * (c - base)) = x;
            }
            __syncthreads();
            if (mine) {
                UhStageReader r{s_stage + 16 * (off - base) + lead};
                UhVerdict v;
                uint32_t *hit = s_hit + tid;
                uh_walk<uint32_t>(r, uh, v, [&](uint32_t kk, uint32_t kp, uint32_t kl, uint32_t vkp, uint32_t, uint32_t, uint32_t) {
                    uh_match(keys, r, hit, kk, kp, kl, vkp);
                });
                present = uh_store(keys, o, i, v, r, hit, true);
                bad = v.kind != IGGY_OK;
            }
            base = hi;
            __syncthreads();  // the stage is free for the next round (or the windows)
        }
        tally(i, valid && !isl, uh > 0, bad, present);

        // the long messages of this wave, one after the other, by the whole wave
        for (uint64_t m = __ballot(valid && isl); m; m &= m - 1) {
            const int l = __ffsll((long long)m) - 1;
            const uint64_t g = __shfl((unsigned long long)(uintptr_t)src, l);
            const uint32_t ln = __shfl(uh, l);
            const uint64_t mi = __shfl((unsigned long long)i, l);
            UhWindowReader r{(const uint8_t *)(uintptr_t)(g & ~15ull), (uint32_t)(g & 15), ln, s_stage + wave * kUhWin};
            UhVerdict v;
            uint32_t *hit = s_hit + 64 * wave + l;  // (every lane writes the same words)
            uh_walk<uint32_t>(r, ln, v, [&](uint32_t kk, uint32_t kp, uint32_t kl, uint32_t vkp, uint32_t, uint32_t, uint32_t) {
                uh_match(keys, r, hit, kk, kp, kl, vkp);
            });
            const uint32_t p = uh_store(keys, o, mi, v, r, hit, lane == 0);
            tally(mi, lane == 0, true, v.kind != IGGY_OK, p);
        }
    }
    if (lane == 0) {
        if (c_with) atomicAdd((unsigned long long *)&res->with_headers, c_with);
        if (c_invalid) {
            atomicAdd((unsigned long long *)&res->invalid_messages, c_invalid);
            atomicMin((unsigned long long *)&res->first_invalid, c_first);
        }
#pragma unroll
        for (uint32_t k = 0; k < IGGY_HEADER_MAX_KEYS; ++k)
            if (k < keys.nkeys && c_found[k]) atomicAdd((unsigned long long *)&res->found[k], c_found[k]);
    }
}

}  // namespace iggy

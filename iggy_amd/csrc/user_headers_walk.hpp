// user_headers_walk.hpp -- the user-header TLV walk, shared by the device kernel
// (user_headers.hip) and the host twin (user_headers.cpp) so both give one verdict.
//
// One pass restates the reference's two stages (include/iggy_codec.h "user headers"):
// validate_user_headers (binary_protocol/src/primitives/user_headers.rs:84-139) over the
// whole buffer, then headers_from_validated_slice with UnknownKinds::Reject
// (common/src/wire_conversions.rs:802-840). A structural error ends the walk at once and
// wins; the first domain error is kept while the structural walk goes on behind it.
#pragma once
#include <stdint.h>

#include "../../include/iggy_codec.h"

#if defined(__HIPCC__)
#define IGGY_UH_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define IGGY_UH_HD inline
#endif

namespace iggy {

constexpr uint32_t kUhMaxField = 255;  // MAX_FIELD_LENGTH, user_headers.rs:38

// HeaderKind::expected_size (common/src/types/message/user_headers.rs:272-281) by kind
// code (:231-247): 0 = any length (Raw, String), else the size. Codes outside 1..15: 0.
IGGY_UH_HD uint32_t uh_fixed_size(uint32_t kind) {
    // one nibble per code: 0 = variable, n = 1 << (n - 1) bytes
    constexpr uint64_t t = (1ull << 12) | (1ull << 16) | (2ull << 20) | (3ull << 24) | (4ull << 28) | (5ull << 32) |
                           (1ull << 36) | (2ull << 40) | (3ull << 44) | (4ull << 48) | (5ull << 52) | (3ull << 56) |
                           (4ull << 60);
    if (kind < 1 || kind > 15) return 0;
    const uint32_t n = (uint32_t)(t >> (4 * kind)) & 15u;
    return n ? 1u << (n - 1) : 0u;
}
IGGY_UH_HD bool uh_known_kind(uint32_t kind) { return kind >= 1 && kind <= 15; }

// a request key as the entry points accept it
IGGY_UH_HD bool uh_key_ok(uint32_t kind, uint32_t length) {
    if (!uh_known_kind(kind) || length == 0 || length > kUhMaxField) return false;
    const uint32_t fx = uh_fixed_size(kind);
    return fx == 0 || fx == length;
}

struct UhVerdict {
    uint32_t kind, reason, offset, detail;  // iggy_header_status
    uint32_t pairs;                         // 0 on any error
};

// R: b(pos) = byte pos of the buffer; ensure(pos, n) makes [pos, pos + n) readable (clipped
// to the buffer). P: the position type (u32 on the device, u64 on the host).
// on_pair(key_kind, key_pos, key_len, value_kind_pos, value_kind, value_pos, value_len) is
// called for every pair that passes the domain stage, in walk order, until the first
// domain error; what it gathered counts only if the verdict is IGGY_OK.
template <class P, class R, class F>
IGGY_UH_HD void uh_walk(R &r, P len, UhVerdict &v, F &&on_pair) {
    v = UhVerdict{IGGY_OK, 0, 0, 0, 0};
    uint32_t dk = IGGY_OK, dreason = 0, doff = 0;  // the first domain error
    P pos = 0, pair_start = 0, key_pos = 0;
    uint32_t tlvs = 0, key_kind = 0, key_len = 0;
    while (pos < len) {
        r.ensure(pos, (P)5);
        const uint32_t kind = r.b(pos);
        if (kind == 0) {
            v = UhVerdict{IGGY_ERR_VALIDATION, IGGY_V_HEADER_KIND_ZERO, (uint32_t)pos, 0, 0};
            return;
        }
        const P lpos = pos + 1;
        if (len - lpos < 4) {
            v = UhVerdict{IGGY_ERR_UNEXPECTED_EOF, 0, (uint32_t)lpos, 4, 0};
            return;
        }
        const uint32_t length = (uint32_t)r.b(lpos) | ((uint32_t)r.b(lpos + 1) << 8) | ((uint32_t)r.b(lpos + 2) << 16) |
                                ((uint32_t)r.b(lpos + 3) << 24);
        if (length == 0 || length > kUhMaxField) {
            v = UhVerdict{IGGY_ERR_VALIDATION, IGGY_V_HEADER_FIELD_LENGTH, (uint32_t)lpos, length, 0};
            return;
        }
        const P dpos = lpos + 4;
        if (len - dpos < length) {
            v = UhVerdict{IGGY_ERR_UNEXPECTED_EOF, 0, (uint32_t)dpos, length, 0};
            return;
        }
        if ((tlvs & 1u) == 0) {
            pair_start = pos;
            key_kind = kind;
            key_pos = dpos;
            key_len = length;
        } else if (dk == IGGY_OK) {
            if (!uh_known_kind(key_kind)) {
                dk = IGGY_ERR_INVALID_HEADER_KIND, dreason = key_kind, doff = (uint32_t)pair_start;
            } else if (!uh_known_kind(kind)) {
                dk = IGGY_ERR_INVALID_HEADER_KIND, dreason = kind, doff = (uint32_t)pair_start;
            } else if (uh_fixed_size(key_kind) && uh_fixed_size(key_kind) != key_len) {
                dk = IGGY_ERR_INVALID_HEADER_KEY, doff = (uint32_t)pair_start;
            } else if (uh_fixed_size(kind) && uh_fixed_size(kind) != length) {
                dk = IGGY_ERR_INVALID_HEADER_VALUE, doff = (uint32_t)pair_start;
            } else {
                r.ensure(pair_start, (P)(dpos + length - pair_start));
                on_pair(key_kind, key_pos, key_len, pos, kind, dpos, length);
            }
        }
        pos = dpos + length;
        ++tlvs;
    }
    if (tlvs & 1u) {
        v = UhVerdict{IGGY_ERR_VALIDATION, IGGY_V_HEADER_ODD_ENTRIES, 0, tlvs, 0};
        return;
    }
    if (dk != IGGY_OK) {
        v = UhVerdict{dk, dreason, doff, 0, 0};
        return;
    }
    v.pairs = tlvs / 2;
}

}  // namespace iggy

// select_clause.hpp -- the select's clause program: the synchronous checks of an
// iggy_select_spec and the truth of its clauses for one message, shared by the device
// kernel (select.hip, k_sel_flags) and the host twin (select.cpp) so both give one verdict.
//
// The semantics are the library's own (include/iggy_codec.h "select"): the reference has
// typed header accessors (common/src/types/message/user_headers.rs) but no ordering.
// Every compare is integer work on bit patterns: floats are ordered through a
// sign-magnitude -> ordered-key map, so no float instruction (and no denormal mode) can
// change a verdict.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/iggy_codec.h"

#if defined(__HIPCC__)
#define IGGY_SEL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define IGGY_SEL_HD inline
#endif

namespace iggy {

typedef uint64_t sel_u64_ua __attribute__((aligned(1), may_alias));

// one clause as the evaluation takes it: the operand normalised once (sel_norm), the
// column pointers flat
struct SelClause {
    uint32_t source, op, kind, length;
    uint64_t lo, hi;
    const uint8_t *kinds, *lengths, *values16;
    const iggy_header_status *status;
};

struct SelProgram {  // travels by value with the launch
    uint32_t n, _pad;
    const uint8_t *mask;
    SelClause c[IGGY_SELECT_MAX_CLAUSES];
};

// fixed size of a header value kind (HeaderKind::expected_size), 0 = Raw / String
IGGY_SEL_HD uint32_t sel_kind_size(uint32_t kind) {
    switch (kind) {
        case 3: case 4: case 9: return 1;
        case 5: case 10: return 2;
        case 6: case 11: case 14: return 4;
        case 7: case 12: case 15: return 8;
        case 8: case 13: return 16;
        default: return 0;
    }
}

// the low `len` (1..16) bytes of a little-endian 128-bit value
IGGY_SEL_HD void sel_mask(uint32_t len, uint64_t &lo, uint64_t &hi) {
    if (len < 8) lo &= (1ull << (8 * len)) - 1;
    if (len <= 8) hi = 0;
    else if (len < 16) hi &= (1ull << (8 * (len - 8))) - 1;
}

// A header value of `kind` in its first `len` bytes -> a pair that orders as the value does
// under an unsigned 128-bit compare. Signed integers: sign-extended, top bit flipped.
// Floats: lo = the ordered key of the bit pattern (-0 as +0), hi = 1 for a NaN.
IGGY_SEL_HD void sel_norm(uint32_t kind, uint32_t len, uint64_t &lo, uint64_t &hi) {
    sel_mask(len, lo, hi);
    if (kind >= 4 && kind <= 8) {
        if (len < 8) {
            const bool neg = (lo >> (8 * len - 1)) & 1;
            if (neg) lo |= ~0ull << (8 * len);
            hi = neg ? ~0ull : 0;
        } else if (len == 8) {
            hi = (lo >> 63) ? ~0ull : 0;
        }
        hi ^= 1ull << 63;
    } else if (kind == 14) {
        uint32_t b = (uint32_t)lo;
        const bool nan = (b & 0x7FFFFFFFu) > 0x7F800000u;
        if ((b & 0x7FFFFFFFu) == 0) b = 0;
        lo = (b >> 31) ? (uint32_t)~b : (b | 0x80000000u);
        hi = nan ? 1 : 0;
    } else if (kind == 15) {
        uint64_t b = lo;
        const bool nan = (b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
        if ((b & 0x7FFFFFFFFFFFFFFFull) == 0) b = 0;
        lo = (b >> 63) ? ~b : (b | (1ull << 63));
        hi = nan ? 1 : 0;
    }
}

IGGY_SEL_HD bool sel_cmp(uint32_t op, uint64_t alo, uint64_t ahi, uint64_t blo, uint64_t bhi) {
    const bool eq = alo == blo && ahi == bhi;
    const bool lt = ahi < bhi || (ahi == bhi && alo < blo);
    switch (op) {
        case IGGY_OP_EQ: return eq;
        case IGGY_OP_NE: return !eq;
        case IGGY_OP_LT: return lt;
        case IGGY_OP_LE: return lt || eq;
        case IGGY_OP_GT: return !(lt || eq);
        default: return !lt;  // IGGY_OP_GE
    }
}

// the truth of clause c for message i of s (pointers of one memory space: all host or all device)
IGGY_SEL_HD bool sel_clause_true(const SelClause &c, const iggy_unpacked_messages &s, uint64_t i) {
    switch (c.source) {
        case IGGY_SEL_OFFSET: return sel_cmp(c.op, s.offsets[i], 0, c.lo, 0);
        case IGGY_SEL_TIMESTAMP: return sel_cmp(c.op, s.timestamps[i], 0, c.lo, 0);
        case IGGY_SEL_ORIGIN_TIMESTAMP: return sel_cmp(c.op, s.origin_timestamps[i], 0, c.lo, 0);
        case IGGY_SEL_PAYLOAD_LENGTH: return sel_cmp(c.op, s.payload_lengths[i], 0, c.lo, 0);
        case IGGY_SEL_USER_HEADERS_LENGTH: return sel_cmp(c.op, s.user_headers_lengths[i], 0, c.lo, 0);
        case IGGY_SEL_ID: return sel_cmp(c.op, s.ids[2 * i], s.ids[2 * i + 1], c.lo, c.hi);
        case IGGY_SEL_HEADER_STATUS: return c.status[i].kind == IGGY_OK;
        default: break;  // IGGY_SEL_HEADER
    }
    const uint32_t k = c.kinds[i];
    if (c.op == IGGY_OP_PRESENT) return k != 0;
    if (c.op == IGGY_OP_ABSENT) return k == 0;
    if (k != c.kind) return false;  // absent, or another kind: false under every compare op
    uint64_t lo = *(const sel_u64_ua *)(c.values16 + 16 * i), hi = *(const sel_u64_ua *)(c.values16 + 16 * i + 8);
    if (k <= 2) {  // Raw, String: equal = same length and the same first `length` bytes
        sel_mask(c.length, lo, hi);
        const bool eq = c.lengths[i] == c.length && lo == c.lo && hi == c.hi;
        return c.op == IGGY_OP_EQ ? eq : !eq;
    }
    sel_norm(k, c.length, lo, hi);
    if (k >= 14) {
        if (hi | c.hi) return c.op == IGGY_OP_NE;  // a NaN on either side
        return sel_cmp(c.op, lo, 0, c.lo, 0);
    }
    return sel_cmp(c.op, lo, hi, c.lo, c.hi);
}

IGGY_SEL_HD bool sel_keep(const SelProgram &p, const iggy_unpacked_messages &s, uint64_t i) {
    bool keep = !p.mask || p.mask[i] != 0;
    for (uint32_t k = 0; k < IGGY_SELECT_MAX_CLAUSES; ++k)
        if (k < p.n && keep) keep = sel_clause_true(p.c[k], s, i);
    return keep;
}

// The synchronous checks of a spec against its source (what both entry points refuse with
// IGGY_ERR_INVALID_ARGUMENT) and the program the evaluation runs. Host code.
inline int sel_prepare(const iggy_select_spec *spec, const iggy_unpacked_messages *src, SelProgram &p) {
    if (!spec || !src || spec->nclauses > IGGY_SELECT_MAX_CLAUSES) return IGGY_ERR_INVALID_ARGUMENT;
    memset(&p, 0, sizeof p);
    p.n = spec->nclauses;
    p.mask = spec->d_mask;
    for (uint32_t k = 0; k < spec->nclauses; ++k) {
        const iggy_select_clause &q = spec->clauses[k];
        SelClause &c = p.c[k];
        c.source = q.source;
        c.op = q.op;
        uint64_t lo, hi;
        memcpy(&lo, q.operand, 8);
        memcpy(&hi, q.operand + 8, 8);
        const bool compare = q.op >= IGGY_OP_EQ && q.op <= IGGY_OP_GE;
        const void *need = nullptr;
        uint32_t width = 16;
        switch (q.source) {
            case IGGY_SEL_OFFSET: need = src->offsets, width = 8; break;
            case IGGY_SEL_TIMESTAMP: need = src->timestamps, width = 8; break;
            case IGGY_SEL_ORIGIN_TIMESTAMP: need = src->origin_timestamps, width = 8; break;
            case IGGY_SEL_PAYLOAD_LENGTH: need = src->payload_lengths, width = 4; break;
            case IGGY_SEL_USER_HEADERS_LENGTH: need = src->user_headers_lengths, width = 4; break;
            case IGGY_SEL_ID: need = src->ids; break;
            case IGGY_SEL_HEADER_STATUS:  // no op, no operand
                if (!q.status) return IGGY_ERR_INVALID_ARGUMENT;
                c.op = 0;
                c.status = q.status;
                continue;
            case IGGY_SEL_HEADER: {
                if (!q.column.value_kinds) return IGGY_ERR_INVALID_ARGUMENT;
                c.kinds = q.column.value_kinds;
                if (q.op == IGGY_OP_PRESENT || q.op == IGGY_OP_ABSENT) continue;
                if (!compare || q.kind < 1 || q.kind > 15 || !q.column.values16) return IGGY_ERR_INVALID_ARGUMENT;
                const uint32_t fx = sel_kind_size(q.kind);
                const bool eq_only = q.kind <= 3;  // Raw, String, Bool
                if (fx ? q.length != fx : (q.length < 1 || q.length > 16)) return IGGY_ERR_INVALID_ARGUMENT;
                if (eq_only && q.op != IGGY_OP_EQ && q.op != IGGY_OP_NE) return IGGY_ERR_INVALID_ARGUMENT;
                if (!fx && !q.column.value_lengths) return IGGY_ERR_INVALID_ARGUMENT;
                c.kind = q.kind;
                c.length = q.length;
                c.lengths = q.column.value_lengths;
                c.values16 = q.column.values16;
                sel_norm(q.kind, q.length, lo, hi);
                c.lo = lo;
                c.hi = hi;
                continue;
            }
            default: return IGGY_ERR_INVALID_ARGUMENT;
        }
        if (!compare || !need) return IGGY_ERR_INVALID_ARGUMENT;  // (PRESENT / ABSENT: headers only)
        sel_mask(width, lo, hi);
        c.lo = lo;
        c.hi = hi;
    }
    return 0;
}

}  // namespace iggy

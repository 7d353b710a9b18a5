// route_key.hpp -- the route's key program: the synchronous checks of an iggy_route_spec
// and the partition of one message, shared by the device kernel (route.hip, k_route_keys)
// and the host twin (route.cpp) so both give one verdict.
//
// The rule is the reference's (include/iggy_codec.h "route"): calculate_32(key) %
// partition_count (core/common/src/utils/hash.rs:18-22; SDK side
// core/common/src/traits/binary_impls/messages.rs:154-164; server side
// core/metadata/src/stm/stream.rs:1303-1324), the key forms of
// core/common/src/types/message/partitioning.rs:84-128.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/iggy_codec.h"
#include "xxh32.hpp"

namespace iggy {

struct RouteProgram {  // travels by value with the launch
    uint32_t partitions, key_source, absent_partition, key_length;
    uint64_t key_stride;
    const uint8_t *keys;
    const uint32_t *partition_ids;
    const uint8_t *kinds, *lengths;
    const uint32_t *pos;
    const uint8_t *mask;
};

// The partition of message i of s, or IGGY_ROUTE_DROP (pointers of one memory space: all
// host or all device). Every key byte is read inside [key, key + length).
IGGY_XXH32_HD uint32_t route_partition(const RouteProgram &p, const iggy_unpacked_messages &s, uint64_t i) {
    if (p.mask && p.mask[i] == 0) return IGGY_ROUTE_DROP;
    uint32_t h;
    switch (p.key_source) {
        case IGGY_ROUTE_KEY_PARTITION: {
            const uint32_t v = p.partition_ids[i];
            return v < p.partitions ? v : IGGY_ROUTE_DROP;
        }
        case IGGY_ROUTE_KEY_ID:
            h = xxh32(Xxh32Reg128{s.ids[2 * i], s.ids[2 * i + 1]}, 16, 0);
            break;
        case IGGY_ROUTE_KEY_BYTES:
            h = xxh32(Xxh32Mem{p.keys + i * p.key_stride}, p.key_length, 0);
            break;
        default: {  // IGGY_ROUTE_KEY_HEADER
            const uint64_t b = s.user_headers_starts[i], e = s.user_headers_starts[i + 1];
            const uint64_t at = p.pos[i], len = p.lengths[i];
            // absent (or invalid headers), or a column that does not describe this message's bytes
            if (p.kinds[i] == 0 || len == 0 || e < b || at + len > e - b) return p.absent_partition;
            h = xxh32(Xxh32Mem{s.user_headers + b + at}, len, 0);
            break;
        }
    }
    return h % p.partitions;
}

// The synchronous checks of a spec against its source (what both entry points refuse with
// IGGY_ERR_INVALID_ARGUMENT) and the program the evaluation runs. Host code.
inline int route_prepare(const iggy_route_spec *spec, const iggy_unpacked_messages *src, RouteProgram &p) {
    if (!spec || !src) return IGGY_ERR_INVALID_ARGUMENT;
    memset(&p, 0, sizeof p);
    if (spec->partitions < 1 || spec->partitions > IGGY_ROUTE_MAX_PARTITIONS) return IGGY_ERR_INVALID_ARGUMENT;
    p.partitions = spec->partitions;
    p.key_source = spec->key_source;
    p.absent_partition = IGGY_ROUTE_DROP;
    p.mask = spec->d_mask;
    if (spec->absent_partition != IGGY_ROUTE_DROP && spec->absent_partition >= spec->partitions)
        return IGGY_ERR_INVALID_ARGUMENT;
    switch (spec->key_source) {
        case IGGY_ROUTE_KEY_ID:
            if (!src->ids) return IGGY_ERR_INVALID_ARGUMENT;
            break;
        case IGGY_ROUTE_KEY_HEADER:
            if (!spec->column.value_kinds || !spec->column.value_lengths || !spec->column.value_pos ||
                !src->user_headers_starts || !src->user_headers)
                return IGGY_ERR_INVALID_ARGUMENT;
            p.absent_partition = spec->absent_partition;
            p.kinds = spec->column.value_kinds;
            p.lengths = spec->column.value_lengths;
            p.pos = spec->column.value_pos;
            break;
        case IGGY_ROUTE_KEY_BYTES:
            if (!spec->d_keys || spec->key_length < 1 || spec->key_length > 255 || spec->key_stride < spec->key_length)
                return IGGY_ERR_INVALID_ARGUMENT;
            p.keys = spec->d_keys;
            p.key_length = spec->key_length;
            p.key_stride = spec->key_stride;
            break;
        case IGGY_ROUTE_KEY_PARTITION:
            if (!spec->d_partition_ids) return IGGY_ERR_INVALID_ARGUMENT;
            p.partition_ids = spec->d_partition_ids;
            break;
        default: return IGGY_ERR_INVALID_ARGUMENT;
    }
    return 0;
}

}  // namespace iggy

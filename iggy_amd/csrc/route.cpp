// route.cpp -- host side of the route: iggy_xxh32 (the reference's calculate_32 is
// iggy_xxh32(key, len, 0)) and iggy_route_partitions_host, the host twin of the device
// route's key stage (route.hip, k_route_keys): the partition per message over HOST arrays,
// with the synchronous refusals of iggy_codec_route_messages_device for the spec. For the
// Rust shim's calculate_32 call sites, small host-side producers, and to pin the hash and
// the partition rule without a GPU.
//
// Pure C++ (no HIP): part of libiggy_codec.so, and builds alone with g++ for the host
// sanitizer run (tests/fuzz/route_host_fuzz.cpp).
#include "route_key.hpp"

extern "C" {

uint32_t iggy_xxh32(const void *data, uint64_t len, uint32_t seed) {
    return iggy::xxh32(iggy::Xxh32Mem{(const uint8_t *)data}, len, seed);
}

int iggy_route_partitions_host(const iggy_unpacked_messages *src, uint64_t count, const iggy_route_spec *spec,
                               uint32_t *partition_of_out) {
    if (!src || !spec || !partition_of_out || count > src->cap_messages) return IGGY_ERR_INVALID_ARGUMENT;
    iggy::RouteProgram p;
    if (int r = iggy::route_prepare(spec, src, p)) return r;
    for (uint64_t i = 0; i < count; ++i) partition_of_out[i] = iggy::route_partition(p, *src, i);
    return 0;
}

}  // extern "C"

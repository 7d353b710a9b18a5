// select.cpp -- host twin of the device select's clause evaluation (select.hip,
// k_sel_flags): iggy_select_mask_host, the keep verdict per message over HOST arrays, with
// the synchronous refusals of iggy_codec_select_messages_device. For small host-side
// consumers, and to pin the clause semantics without a GPU.
//
// Pure C++ (no HIP): part of libiggy_codec.so, and builds alone with g++ for the host
// sanitizer run (tests/fuzz/select_host_fuzz.cpp).
#include "select_clause.hpp"

extern "C" {

int iggy_select_mask_host(const iggy_unpacked_messages *src, uint64_t count, const iggy_select_spec *spec,
                          uint8_t *keep_out) {
    if (!src || !spec || !keep_out || count > src->cap_messages) return IGGY_ERR_INVALID_ARGUMENT;
    iggy::SelProgram p;
    if (int r = iggy::sel_prepare(spec, src, p)) return r;
    for (uint64_t i = 0; i < count; ++i) keep_out[i] = iggy::sel_keep(p, *src, i) ? 1 : 0;
    return 0;
}

}  // extern "C"

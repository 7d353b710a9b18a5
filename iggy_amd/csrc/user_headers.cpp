// user_headers.cpp -- host twin of the device user-header kernel (user_headers.hip):
// iggy_user_headers_validate / iggy_user_headers_get, the verdicts of
// validate_user_headers (binary_protocol/src/primitives/user_headers.rs:84-139) and
// headers_from_validated_slice (common/src/wire_conversions.rs:802-840) for a host-side
// consumer (IggyMessage::get_user_header) and for records too small to be worth a launch.
//
// Pure C++ (no HIP): part of libiggy_codec.so, and builds alone with g++ for the host
// sanitizer run (tests/fuzz/user_headers_host_fuzz.cpp).
#include <string.h>

#include "user_headers_walk.hpp"

namespace {

struct HostReader {
    const uint8_t *p;
    uint8_t b(uint64_t pos) const { return p[pos]; }
    void ensure(uint64_t, uint64_t) const {}
};

void put_status(iggy_header_status *st, const iggy::UhVerdict &v) {
    if (!st) return;
    st->kind = v.kind;
    st->reason = v.reason;
    st->offset = v.offset;
    st->detail = v.detail;
}

}  // namespace

extern "C" {

int iggy_user_headers_validate(const uint8_t *buf, uint64_t len, uint32_t *pairs, iggy_header_status *st) {
    iggy::UhVerdict v{};
    if (!buf && len) {
        v.kind = IGGY_ERR_INVALID_ARGUMENT;
    } else {
        HostReader r{buf};
        iggy::uh_walk<uint64_t>(r, len, v, [](uint32_t, uint64_t, uint32_t, uint64_t, uint32_t, uint64_t, uint32_t) {});
    }
    if (pairs) *pairs = v.pairs;
    put_status(st, v);
    return (int)v.kind;
}

int iggy_user_headers_get(const uint8_t *buf, uint64_t len, const iggy_header_key *key, uint8_t *value_kind,
                          uint32_t *value_pos, uint8_t *value_len, iggy_header_status *st) {
    iggy::UhVerdict v{};
    uint32_t vk = 0, vl = 0;
    uint64_t vp = 0;
    if ((!buf && len) || !key || !iggy::uh_key_ok(key->kind, key->length)) {
        v.kind = IGGY_ERR_INVALID_ARGUMENT;
    } else {
        HostReader r{buf};
        iggy::uh_walk<uint64_t>(r, len, v,
                                [&](uint32_t kk, uint64_t kp, uint32_t kl, uint64_t, uint32_t k, uint64_t p, uint32_t l) {
                                    if (kk != key->kind || kl != key->length || memcmp(buf + kp, key->bytes, kl) != 0)
                                        return;
                                    vk = k, vp = p, vl = l;  // BTreeMap::insert: the last pair wins
                                });
        if (v.kind != IGGY_OK) vk = 0, vp = 0, vl = 0;
    }
    if (value_kind) *value_kind = (uint8_t)vk;
    if (value_pos) *value_pos = (uint32_t)vp;
    if (value_len) *value_len = (uint8_t)vl;
    put_status(st, v);
    return (int)v.kind;
}

}  // extern "C"

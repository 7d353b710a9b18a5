// Host sanitizer harness (TEST INFRASTRUCTURE): iggy_amd/csrc/user_headers.cpp alone
// under g++ -fsanitize=address,undefined, driven by tests/test_user_headers_fuzz_cpu.py,
// which feeds seeded random and truncated buffers on stdin. One command per line:
//   V <hex|->                     iggy_user_headers_validate
//   G <kind> <keyhex> <hex|->     iggy_user_headers_get
// Every buffer is copied into a heap block of exactly its length, so a read past its end
// is an AddressSanitizer report. Every out-parameter is checked to lie inside the buffer
// (exit 3 otherwise); one result line per command for the comparison with the restatement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/iggy_codec.h"

static std::vector<uint8_t> unhex(const char *h) {
    std::vector<uint8_t> v;
    if (!h || h[0] == '-') return v;
    const size_t n = strlen(h);
    for (size_t i = 0; i + 1 < n; i += 2) {
        unsigned x = 0;
        sscanf(h + i, "%2x", &x);
        v.push_back((uint8_t)x);
    }
    return v;
}

static void fail(const char *what, const char *line) {
    fprintf(stderr, "out of bounds: %s in %s\n", what, line);
    exit(3);
}

// the status stays inside a buffer of len bytes
static void check_status(const iggy_header_status &st, uint64_t len, const char *line) {
    if (st.kind == IGGY_OK && (st.reason || st.offset || st.detail)) fail("ok status not zero", line);
    if (st.offset > len) fail("offset", line);
    if (st.kind == IGGY_ERR_UNEXPECTED_EOF && (uint64_t)st.offset + st.detail <= len) fail("eof that fits", line);
}

int main() {
    char *line = nullptr;
    size_t cap = 0;
    ssize_t got;
    while ((got = getline(&line, &cap, stdin)) > 0) {
        std::string keep(line);
        char *save = nullptr;
        char *cmd = strtok_r(line, " \n", &save);
        if (!cmd) continue;
        if (cmd[0] == 'V') {
            const std::vector<uint8_t> v = unhex(strtok_r(nullptr, " \n", &save));
            uint8_t *buf = (uint8_t *)malloc(v.size() ? v.size() : 1);
            if (!v.empty()) memcpy(buf, v.data(), v.size());
            uint32_t pairs = 0xDEADBEEF;
            iggy_header_status st;
            memset(&st, 0xEE, sizeof st);
            const int rc = iggy_user_headers_validate(v.empty() ? nullptr : buf, v.size(), &pairs, &st);
            if ((uint32_t)rc != st.kind) fail("rc", keep.c_str());
            check_status(st, v.size(), keep.c_str());
            if ((uint64_t)pairs * 12 > v.size() || (st.kind != IGGY_OK && pairs)) fail("pairs", keep.c_str());
            // null out-parameters are legal
            if (iggy_user_headers_validate(v.empty() ? nullptr : buf, v.size(), nullptr, nullptr) != rc)
                fail("rc without out-parameters", keep.c_str());
            printf("V %u %u %u %u %u\n", st.kind, st.reason, st.offset, st.detail, pairs);
            free(buf);
        } else if (cmd[0] == 'G') {
            const unsigned kind = (unsigned)strtoul(strtok_r(nullptr, " \n", &save), nullptr, 10);
            const std::vector<uint8_t> kb = unhex(strtok_r(nullptr, " \n", &save));
            const std::vector<uint8_t> v = unhex(strtok_r(nullptr, " \n", &save));
            iggy_header_key *key = (iggy_header_key *)calloc(1, sizeof(iggy_header_key));
            key->kind = (uint8_t)kind;
            key->length = (uint8_t)kb.size();
            if (!kb.empty()) memcpy(key->bytes, kb.data(), kb.size() < 255 ? kb.size() : 255);
            uint8_t *buf = (uint8_t *)malloc(v.size() ? v.size() : 1);
            if (!v.empty()) memcpy(buf, v.data(), v.size());
            uint8_t vk = 0xEE, vl = 0xEE;
            uint32_t vp = 0xDEADBEEF;
            iggy_header_status st;
            memset(&st, 0xEE, sizeof st);
            const int rc = iggy_user_headers_get(v.empty() ? nullptr : buf, v.size(), key, &vk, &vp, &vl, &st);
            if ((uint32_t)rc != st.kind) fail("rc", keep.c_str());
            if (rc != IGGY_ERR_INVALID_ARGUMENT) check_status(st, v.size(), keep.c_str());
            if (vk ? (vl == 0 || (uint64_t)vp + vl > v.size() || vp < 10) : (vl != 0 || vp != 0)) fail("value", keep.c_str());
            if (st.kind != IGGY_OK && vk) fail("value of invalid headers", keep.c_str());
            printf("G %u %u %u %u %u %u %u\n", st.kind, st.reason, st.offset, st.detail, vk, vp, vl);
            free(buf);
            free(key);
        }
    }
    free(line);
    return 0;
}

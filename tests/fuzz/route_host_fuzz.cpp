// Host sanitizer harness (TEST INFRASTRUCTURE): iggy_amd/csrc/route.cpp alone under
// g++ -fsanitize=address,undefined, driven by tests/test_route_fuzz_cpu.py, which feeds
// seeded sources and specs on stdin. One command per line:
//   N <count>                       a new source of <count> messages (forgets every array)
//   A <name> <offset> <hex|->       one array (ids, user_headers_starts, user_headers, keys,
//                                   partition_ids, value_kinds, value_lengths, value_pos,
//                                   mask); "-" = NULL
//   H <offset> <hex>                iggy_xxh32 of the bytes, seed 0 -> one line "<hash>"
//   Q <partitions> <key source> <absent> <key length> <key stride>
// Every array is copied into a heap block of exactly <offset> + its length bytes and starts
// <offset> bytes in, so it ENDS at the block's last byte at any alignment 0..15 of its
// first: a read past a key's (or an array's) end is an AddressSanitizer report. The
// partitions land in a block of exactly <count> entries. One result line per Q
// ("<rc> <partition ...|->") for the comparison with the restatement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../include/iggy_codec.h"

struct Block {
    uint8_t *base = nullptr, *p = nullptr;
    size_t n = 0;
    void set(size_t off, const char *h) {
        free(base);
        base = p = nullptr;
        n = 0;
        if (!h || h[0] == '-') return;
        n = strlen(h) / 2;
        base = (uint8_t *)malloc(off + n ? off + n : 1);
        p = base + off;
        for (size_t i = 0; i < n; ++i) {
            unsigned x = 0;
            sscanf(h + 2 * i, "%2x", &x);
            p[i] = (uint8_t)x;
        }
    }
    ~Block() { free(base); }
};

int main() {
    char *line = nullptr;
    size_t cap = 0;
    uint64_t count = 0;
    Block ids, uhs, uh, keys, pids, kinds, lengths, pos, mask, one;
    Block *all[] = {&ids, &uhs, &uh, &keys, &pids, &kinds, &lengths, &pos, &mask};
    const char *names[] = {"ids", "user_headers_starts", "user_headers", "keys", "partition_ids",
                           "value_kinds", "value_lengths", "value_pos", "mask"};
    while (getline(&line, &cap, stdin) > 0) {
        char *save = nullptr;
        char *cmd = strtok_r(line, " \n", &save);
        if (!cmd) continue;
        auto tok = [&]() { return strtok_r(nullptr, " \n", &save); };
        if (cmd[0] == 'N') {
            count = strtoull(tok(), nullptr, 10);
            for (Block *b : all) b->set(0, nullptr);
        } else if (cmd[0] == 'A') {
            const std::string name = tok();
            Block *b = nullptr;
            for (int k = 0; k < 9; ++k)
                if (name == names[k]) b = all[k];
            if (!b) return 4;
            const size_t off = strtoull(tok(), nullptr, 10);
            b->set(off, tok());
        } else if (cmd[0] == 'H') {
            const size_t off = strtoull(tok(), nullptr, 10);
            const char *h = tok();
            one.set(off, h && h[0] != '-' ? h : "");
            printf("%u\n", iggy_xxh32(one.p, one.n, 0));
        } else if (cmd[0] == 'Q') {
            iggy_unpacked_messages src;
            memset(&src, 0, sizeof src);
            src.cap_messages = count;
            src.cap_user_headers_bytes = uh.n;
            src.ids = (uint64_t *)ids.p;
            src.user_headers_starts = (uint64_t *)uhs.p;
            src.user_headers = uh.p;
            iggy_route_spec spec;
            memset(&spec, 0, sizeof spec);
            spec.partitions = (uint32_t)strtoul(tok(), nullptr, 10);
            spec.key_source = (uint32_t)strtoul(tok(), nullptr, 10);
            spec.absent_partition = (uint32_t)strtoul(tok(), nullptr, 10);
            spec.key_length = (uint32_t)strtoul(tok(), nullptr, 10);
            spec.key_stride = strtoull(tok(), nullptr, 10);
            spec.d_keys = keys.p;
            spec.d_partition_ids = (const uint32_t *)pids.p;
            spec.column.value_kinds = kinds.p;
            spec.column.value_lengths = lengths.p;
            spec.column.value_pos = (uint32_t *)pos.p;
            spec.d_mask = mask.p;
            uint32_t *part = (uint32_t *)malloc(count ? 4 * count : 1);
            memset(part, 0xEE, count ? 4 * count : 1);
            const int rc = iggy_route_partitions_host(&src, count, &spec, part);
            printf("%d", rc);
            if (rc == 0 && count) {
                for (uint64_t i = 0; i < count; ++i) printf(" %u", part[i]);
            } else {
                for (uint64_t i = 0; rc != 0 && i < count; ++i)
                    if (part[i] != 0xEEEEEEEEu) return 5;  // a refusal writes nothing
                printf(" -");
            }
            printf("\n");
            free(part);
        }
    }
    free(line);
    return 0;
}

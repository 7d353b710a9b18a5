// Host sanitizer harness (TEST INFRASTRUCTURE): iggy_amd/csrc/select.cpp alone under
// g++ -fsanitize=address,undefined, driven by tests/test_select_fuzz_cpu.py, which feeds
// seeded sources and specs on stdin. One command per line:
//   N <count>                               a new source of <count> messages (forgets every array)
//   A <name> <hex|->                        one array of the source (offsets, timestamps,
//                                           origin_timestamps, payload_lengths, user_headers_lengths, ids)
//   C <idx> <kinds hex> <lengths hex> <values16 hex>   header column <idx> (0..3); "-" = NULL
//   T <idx> <hex|->                         status array <idx> (0..3), 16 B per message
//   M <hex|->                               the mask
//   Q <use mask 0/1> <nclauses> {<source> <op> <kind> <length> <operand hex> <column idx|-1> <status idx|-1>}*
// Every array is copied into a heap block of exactly its length, so a read past its end is
// an AddressSanitizer report; the verdicts land in a block of exactly <count> bytes. One
// result line per Q ("<rc> <verdict hex|->") for the comparison with the restatement.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/iggy_codec.h"

struct Block {
    uint8_t *p = nullptr;
    void set(const char *h) {
        free(p);
        p = nullptr;
        if (!h || h[0] == '-') return;
        const size_t n = strlen(h) / 2;
        p = (uint8_t *)malloc(n ? n : 1);
        for (size_t i = 0; i < n; ++i) {
            unsigned x = 0;
            sscanf(h + 2 * i, "%2x", &x);
            p[i] = (uint8_t)x;
        }
    }
    ~Block() { free(p); }
};

int main() {
    char *line = nullptr;
    size_t cap = 0;
    uint64_t count = 0;
    Block offsets, timestamps, origin, plen, uhlen, ids, mask, kinds[4], lengths[4], values[4], status[4];
    while (getline(&line, &cap, stdin) > 0) {
        char *save = nullptr;
        char *cmd = strtok_r(line, " \n", &save);
        if (!cmd) continue;
        auto tok = [&]() { return strtok_r(nullptr, " \n", &save); };
        if (cmd[0] == 'N') {
            count = strtoull(tok(), nullptr, 10);
            for (Block *b : {&offsets, &timestamps, &origin, &plen, &uhlen, &ids, &mask}) b->set(nullptr);
            for (int k = 0; k < 4; ++k) kinds[k].set(nullptr), lengths[k].set(nullptr), values[k].set(nullptr), status[k].set(nullptr);
        } else if (cmd[0] == 'A') {
            const std::string name = tok();
            Block *b = name == "offsets" ? &offsets : name == "timestamps" ? &timestamps
                     : name == "origin_timestamps" ? &origin : name == "payload_lengths" ? &plen
                     : name == "user_headers_lengths" ? &uhlen : name == "ids" ? &ids : nullptr;
            if (!b) return 4;
            b->set(tok());
        } else if (cmd[0] == 'C') {
            const int k = atoi(tok()) & 3;
            kinds[k].set(tok());
            lengths[k].set(tok());
            values[k].set(tok());
        } else if (cmd[0] == 'T') {
            const int k = atoi(tok()) & 3;
            status[k].set(tok());
        } else if (cmd[0] == 'M') {
            mask.set(tok());
        } else if (cmd[0] == 'Q') {
            iggy_unpacked_messages src;
            memset(&src, 0, sizeof src);
            src.cap_messages = count;
            src.offsets = (uint64_t *)offsets.p;
            src.timestamps = (uint64_t *)timestamps.p;
            src.origin_timestamps = (uint64_t *)origin.p;
            src.payload_lengths = (uint32_t *)plen.p;
            src.user_headers_lengths = (uint32_t *)uhlen.p;
            src.ids = (uint64_t *)ids.p;
            iggy_select_spec *spec = (iggy_select_spec *)calloc(1, sizeof(iggy_select_spec));
            const int use_mask = atoi(tok());
            spec->d_mask = use_mask ? mask.p : nullptr;
            spec->nclauses = (uint32_t)atoi(tok());
            for (uint32_t k = 0; k < spec->nclauses && k < IGGY_SELECT_MAX_CLAUSES; ++k) {
                iggy_select_clause &c = spec->clauses[k];
                c.source = (uint32_t)atoi(tok());
                c.op = (uint32_t)atoi(tok());
                c.kind = (uint8_t)atoi(tok());
                c.length = (uint8_t)atoi(tok());
                Block operand;
                const char *h = tok();
                operand.set(h);
                const size_t on = h && h[0] != '-' ? strlen(h) / 2 : 0;
                if (on) memcpy(c.operand, operand.p, on < 16 ? on : 16);
                const int col = atoi(tok()), st = atoi(tok());
                if (col >= 0) {
                    c.column.value_kinds = kinds[col & 3].p;
                    c.column.value_lengths = lengths[col & 3].p;
                    c.column.values16 = values[col & 3].p;
                }
                if (st >= 0) c.status = (const iggy_header_status *)status[st & 3].p;
            }
            uint8_t *keep = (uint8_t *)malloc(count ? count : 1);
            memset(keep, 0xEE, count ? count : 1);
            const int rc = iggy_select_mask_host(&src, count, spec, keep);
            printf("%d ", rc);
            if (rc == 0 && count) {
                for (uint64_t i = 0; i < count; ++i) {
                    if (keep[i] > 1) return 3;  // every verdict written, 0 or 1
                    printf("%02x", keep[i]);
                }
            } else {
                for (uint64_t i = 0; rc != 0 && i < count; ++i)
                    if (keep[i] != 0xEE) return 5;  // a refusal writes nothing
                printf("-");
            }
            printf("\n");
            free(keep);
            free(spec);
        }
    }
    free(line);
    return 0;
}

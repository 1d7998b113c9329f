// flow_rules_main.cpp -- pip_amd/csrc/pipck_flow.hpp in its host form, driven by
// tests/test_flow_rules.py.  Plain C++17, nothing of HIP.
//
// Reads one query per line from stdin and prints one line of decimal numbers per
// query (u64 arguments are decimal):
//   def  ORIGIN I NF               implicit_flow
//   walk ORIGIN FIRST STEP NF K    FlowWalk's first K flows, stepped by next()
//   tile ORIGIN TILE NF            TileFlow::flow of lanes 0..63
//   task ORIGIN P0 NF              task_flow of lanes 0..63
//   res  VERIFY P F BAD            packet_result<VERIFY>
//   res4 VERIFY P F BAD            the form that reports on the spot: "value *err" (*err starts at 0)
//   tab  F NF                      flow_pseudo on a 4-entry table {10, 11, 12, 13}: "value bad"
//   err  START REFUSED HAVE        *err after refuse() (HAVE 0: refuse(nullptr), prints START)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../pip_amd/csrc/pipck_flow.hpp"

using namespace pipck;

int main() {
    char op[8];
    unsigned long long a[5];
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        const int got = sscanf(line, "%7s %llu %llu %llu %llu %llu", op, &a[0], &a[1], &a[2], &a[3], &a[4]);
        if (got < 1) continue;
        if (!strcmp(op, "def") && got == 4) {
            printf("%u\n", implicit_flow(a[0], a[1], (uint32_t)a[2]));
        } else if (!strcmp(op, "walk") && got == 6) {
            FlowWalk w(true, (uint64_t)a[0], (uint64_t)a[1], (uint64_t)a[2], (uint32_t)a[3]);
            for (unsigned long long k = 0; k < a[4]; k++, w.next()) printf("%u ", w.flow);
            printf("\n");
        } else if (!strcmp(op, "tile") && got == 4) {
            for (uint32_t l = 0; l < 64; l++) printf("%u ", TileFlow(a[0], a[1], l, (uint32_t)a[2]).flow());
            printf("\n");
        } else if (!strcmp(op, "task") && got == 4) {
            for (uint32_t l = 0; l < 64; l++) printf("%u ", task_flow(a[0], a[1], l, (uint32_t)a[2]));
            printf("\n");
        } else if (!strcmp(op, "res") && got == 5) {
            const uint32_t P = (uint32_t)a[1], F = (uint32_t)a[2];
            printf("%u\n", a[0] ? packet_result<true>(P, F, a[3] != 0) : packet_result<false>(P, F, a[3] != 0));
        } else if (!strcmp(op, "res4") && got == 5) {
            const uint32_t P = (uint32_t)a[1], F = (uint32_t)a[2];
            uint32_t e = 0;
            const uint32_t r = a[0] ? packet_result<true>(P, F, a[3] != 0, &e) : packet_result<false>(P, F, a[3] != 0, &e);
            printf("%u %u\n", r, e);
        } else if (!strcmp(op, "tab") && got == 3) {
            // entries past the fourth sit in no array at all: a read there is a read outside the table
            static const uint32_t table[4] = {10, 11, 12, 13};
            bool bad = false;
            const uint32_t v = flow_pseudo(table, (uint32_t)a[0], (uint32_t)a[1], bad);
            printf("%u %d\n", v, (int)bad);
        } else if (!strcmp(op, "err") && got == 4) {
            uint32_t e = (uint32_t)a[0];
            refuse(a[2] ? &e : nullptr, a[1] != 0);
            printf("%u\n", e);
        } else {
            fprintf(stderr, "bad query: %s", line);
            return 2;
        }
    }
    return 0;
}

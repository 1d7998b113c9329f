// fwd_key_main.cpp -- pip_amd/csrc/pipck_fwdkey.hpp in its host form, driven by
// tests/test_fwd_key_header.py, which builds it with -fsanitize=address,undefined.
// Plain C++17, nothing of HIP.
//
// Reads one query per line from stdin and prints one line per query.  Bytes are
// hex ("-" for none); every frame, key list and table is copied into a heap
// block of exactly its size, so a read past it is an AddressSanitizer report.
//   key    FRAMEHEX                "0" malformed, "1" no key, "2 KEYHEX"
//   hash   KEYHEX                  the hash, decimal
//   build  NSLOTS RULE,RULE,.. KEYSHEX    "STATUS" and, for status 0, " TABLEHEX"
//   lookup NSLOTS TABLEHEX KEYHEX  "1 RULE" or "0"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../pip_amd/csrc/pipck_fwdkey.hpp"

using namespace pipck;

// An exact-size heap copy of the bytes a hex string spells.
struct Bytes {
    size_t n;
    uint8_t* p;  // n == 0: a block of no bytes, which nobody may read
    explicit Bytes(const std::string& hex) : n(hex == "-" ? 0 : hex.size() / 2), p(static_cast<uint8_t*>(malloc(n))) {
        for (size_t i = 0; i < n; i++) p[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
    }
    ~Bytes() { free(p); }
    Bytes(const Bytes&) = delete;
};

static void print_hex(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "key") {
            std::string hex;
            in >> hex;
            const Bytes f(hex);
            uint32_t k[kFwdKeyWords];
            const uint32_t kind = fwdkey_of_frame(f.p, (uint32_t)f.n, k);
            printf("%u", kind);
            if (kind == kFwdKeyed) {
                pipck_fwd_key key;
                fwdkey_from_words(k, key);
                printf(" ");
                print_hex(reinterpret_cast<const uint8_t*>(&key), sizeof key);
            }
            printf("\n");
        } else if (op == "hash") {
            std::string hex;
            in >> hex;
            const Bytes b(hex);
            if (b.n != sizeof(pipck_fwd_key)) return 2;
            uint32_t k[kFwdKeyWords];
            fwdkey_words(*reinterpret_cast<const pipck_fwd_key*>(b.p), k);
            printf("%u\n", fwdkey_hash(k));
        } else if (op == "build") {
            unsigned long long n_slots;
            std::string rules_s, hex;
            in >> n_slots >> rules_s >> hex;
            const Bytes keys(hex);
            std::vector<uint32_t> rules;
            std::istringstream rs(rules_s);
            for (std::string r; std::getline(rs, r, ',');)
                if (r != "-") rules.push_back((uint32_t)strtoul(r.c_str(), nullptr, 10));
            if (keys.n != rules.size() * sizeof(pipck_fwd_key)) return 2;
            // a slot count the builder must refuse gets a one-entry block: refused before it is touched
            const bool ok = fwdkey_table_slots_valid(n_slots);
            const size_t bytes = (ok ? (size_t)n_slots : 1) * sizeof(pipck_fwd_entry);
            pipck_fwd_entry* table = static_cast<pipck_fwd_entry*>(malloc(bytes));
            memset(table, 0xA5, bytes);
            const int rc = fwdkey_table_build(reinterpret_cast<const pipck_fwd_key*>(keys.p), rules.data(), rules.size(),
                                              table, n_slots);
            printf("%d", rc);
            if (rc == 0) {
                printf(" ");
                print_hex(reinterpret_cast<const uint8_t*>(table), bytes);
            }
            printf("\n");
            free(table);
        } else if (op == "lookup") {
            unsigned long long n_slots;
            std::string thex, khex;
            in >> n_slots >> thex >> khex;
            const Bytes t(thex), kb(khex);
            if (t.n != n_slots * sizeof(pipck_fwd_entry) || kb.n != sizeof(pipck_fwd_key) ||
                !fwdkey_table_slots_valid(n_slots))
                return 2;
            uint32_t rule = 0;
            if (fwdkey_lookup_host(reinterpret_cast<const pipck_fwd_entry*>(t.p), n_slots,
                                   *reinterpret_cast<const pipck_fwd_key*>(kb.p), rule))
                printf("1 %u\n", rule);
            else
                printf("0\n");
        } else {
            fprintf(stderr, "bad query: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}

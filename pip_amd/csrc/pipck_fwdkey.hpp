// pipck_fwdkey.hpp -- a frame's flow key, its hash, the probe of a binding table
// and the table's builder: the one definition of each, for the classify kernels
// (pipck_fwdcls.hip), for pipck_fwd_key_hash / pipck_fwd_frame_key /
// pipck_fwd_table_build and for a stand-alone CPU program
// (tests/fwd_key_main.cpp, built with sanitizers by tests/test_fwd_key_header.py).
// Plain integer code: under a plain C++17 compiler it includes nothing of HIP.
//
// The headers are walked by the rules of fwd_parse (pipck_fwdparse.hpp), which
// are those of tx_from_window and rx_from_window.  This file calls none of them
// and none of their helpers, for the reason pipck_fwdparse.hpp gives: a further
// caller changes how the compiler inlines them into the kernels that exist.
//
// A key is handled as its ten little-endian dwords k[0..9] -- the 40 bytes of a
// pipck_fwd_key as memory holds them: k[0..3] src, k[4..7] dst, k[8] the four
// port bytes, k[9] = proto | family << 8 (pad zero).  They are the dwords a
// frame's header holds, so no byte order is ever fixed.
#pragma once
#include <stdint.h>

#include "../../include/pipck.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PIPCK_KEYFN __host__ __device__ __forceinline__
#else
#define PIPCK_KEYFN inline
#endif

namespace pipck {

constexpr int kFwdKeyWords = 10;
constexpr uint32_t kFwdMaxProbe = PIPCK_FWD_MAX_PROBE;
constexpr uint32_t kFwdTagBit = 0x80000000u;
// fwdkey_parse's answers
constexpr uint32_t kFwdKeyMalformed = 0, kFwdKeyNone = 1, kFwdKeyed = 2;

static_assert(sizeof(pipck_fwd_key) == 40 && sizeof(pipck_fwd_entry) == 48, "a key is ten dwords, an entry three chunks");

PIPCK_KEYFN uint32_t fwdkey_rotl(uint32_t x, uint32_t r) { return x << r | x >> (32u - r); }
PIPCK_KEYFN uint32_t fwdkey_be16(uint32_t lo16) { return (lo16 & 0xFFu) << 8 | (lo16 >> 8 & 0xFFu); }

// The hash of include/pipck.h, all arithmetic modulo 2^32.
PIPCK_KEYFN uint32_t fwdkey_hash(const uint32_t (&k)[kFwdKeyWords]) {
    uint32_t x = 0;
    for (int j = 0; j < kFwdKeyWords; j++) x = fwdkey_rotl(x ^ k[j], 13) * 0x9E3779B1u;
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    return x;
}

// One frame's key.  w(j): frame bytes [j, j + 4) as memory's dword, j a multiple
// of 4; it is asked only for j + 4 <= len, so a caller that answers from the
// frame's own bytes reads nothing past them.  len: the frame's bytes.
// kFwdKeyMalformed: step 3 of pipck_fwd_rewrite_ring's list.  kFwdKeyNone: a
// frame whose upper layer is not located, is none of TCP, UDP, ICMP over IPv4,
// ICMPv6 over IPv6, or is too short for its L4 fields.  kFwdKeyed: k is the key.
template <class Words>
PIPCK_KEYFN uint32_t fwdkey_parse(const Words& w, uint32_t len, uint32_t (&k)[kFwdKeyWords]) {
    for (int j = 0; j < kFwdKeyWords; j++) k[j] = 0;
    if (len < 20) return kFwdKeyMalformed;
    const uint32_t w0 = w(0u), b0 = w0 & 0xFFu, ver = b0 >> 4;
    uint32_t ip_end, proto, l4off;
    if (ver == 4) {
        const uint32_t ihl = (b0 & 15u) * 4u, total = fwdkey_be16(w0 >> 16);
        if (ihl < 20 || total < ihl || total > len) return kFwdKeyMalformed;
        ip_end = total;
        if (fwdkey_be16(w(4u) >> 16) & 0x3FFFu) return kFwdKeyNone;  // a fragment
        proto = w(8u) >> 8 & 0xFFu;
        l4off = ihl;
        k[0] = w(12u);
        k[4] = w(16u);
    } else if (ver == 6 && len >= 40) {
        const uint32_t w1 = w(4u);
        const uint32_t plen = fwdkey_be16(w1 & 0xFFFFu);
        if (40 + plen > len) return kFwdKeyMalformed;
        ip_end = 40 + plen;
        // hop-by-hop 0, destination options 60 and atomic fragments 44 are walked, at most 8 of them
        uint32_t nh = w1 >> 16 & 0xFFu, at = 40;
        bool up = false;
        for (int n = 0; n < 9; n++) {
            if (nh != 0 && nh != 60 && nh != 44) {
                up = nh != 43;  // a routing header
                break;
            }
            if (n == 8) break;           // a ninth extension header
            if (at + 8 > ip_end) break;  // does not fit in the payload
            const uint32_t x = w(at);    // next header, length, and a fragment's field
            if (nh == 44) {
                if (fwdkey_be16(x >> 16) & 0xFFF9u) break;  // an offset or M
                at += 8;
            } else {
                at += 8u * ((x >> 8 & 0xFFu) + 1u);
            }
            if (at > ip_end) break;
            nh = x & 0xFFu;
        }
        if (!up) return kFwdKeyNone;
        proto = nh;
        l4off = at;
        for (int j = 0; j < 4; j++) k[j] = w(8u + 4u * j), k[4 + j] = w(24u + 4u * j);
    } else {
        return kFwdKeyMalformed;
    }
    const bool tcpudp = proto == 6u || proto == 17u;
    if (!tcpudp && proto != (ver == 4 ? 1u : 58u)) return kFwdKeyNone;
    if (ip_end - l4off < (proto == 6u ? 20u : 8u)) return kFwdKeyNone;  // no room for the L4 fields
    if (tcpudp) k[8] = w(l4off);  // the four port bytes at message offset 0
    k[9] = proto | ver << 8;
    return kFwdKeyed;
}

// Four dwords of a table entry, as memory holds them.
struct FwdChunk {
    uint32_t x, y, z, w;
};

// The probe of include/pipck.h.  load(i, c): chunk c (0: src, 1: dst, 2: ports,
// proto / family / pad, rule, tag) of entry i.  mask = n_slots - 1, n_slots a
// power of two up to 2^31: every index asked for is below n_slots, and the loop
// ends after kFwdMaxProbe entries whatever the table holds.  The third chunk is
// loaded first and the address chunks only behind a matching tag, so a probe
// that does not match costs one 16-byte load.
template <class Load>
PIPCK_KEYFN bool fwdkey_lookup(const Load& load, uint32_t mask, const uint32_t (&k)[kFwdKeyWords], uint32_t hash,
                               uint32_t& rule) {
    const uint32_t tag = hash | kFwdTagBit;
    for (uint32_t p = 0; p < kFwdMaxProbe; p++) {
        const uint32_t i = (hash + p) & mask;
        const FwdChunk c2 = load(i, 2u);
        if (c2.w == 0u) return false;
        if (c2.w != tag || c2.x != k[8] || c2.y != k[9]) continue;
        const FwdChunk c0 = load(i, 0u), c1 = load(i, 1u);
        if (c0.x == k[0] && c0.y == k[1] && c0.z == k[2] && c0.w == k[3] && c1.x == k[4] && c1.y == k[5] &&
            c1.z == k[6] && c1.w == k[7]) {
            rule = c2.z;
            return true;
        }
    }
    return false;
}

// ---- host side: bytes in ordinary memory ----------------------------------

inline uint32_t fwdkey_le32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
inline void fwdkey_put32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}
inline void fwdkey_words(const pipck_fwd_key& key, uint32_t (&k)[kFwdKeyWords]) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&key);
    for (int j = 0; j < kFwdKeyWords; j++) k[j] = fwdkey_le32(p + 4 * j);
}
inline void fwdkey_from_words(const uint32_t (&k)[kFwdKeyWords], pipck_fwd_key& key) {
    uint8_t* p = reinterpret_cast<uint8_t*>(&key);
    for (int j = 0; j < kFwdKeyWords; j++) fwdkey_put32(p + 4 * j, k[j]);
}

// A frame in host memory: every read is of bytes [j, j + 4), j + 4 <= len.
struct FwdHostWords {
    const uint8_t* p;
    uint32_t operator()(uint32_t j) const { return fwdkey_le32(p + j); }
};
inline uint32_t fwdkey_of_frame(const uint8_t* frame, uint32_t len, uint32_t (&k)[kFwdKeyWords]) {
    return fwdkey_parse(FwdHostWords{frame}, len, k);
}

// A table in host memory.
struct FwdHostTable {
    const pipck_fwd_entry* t;
    FwdChunk operator()(uint32_t i, uint32_t c) const {
        const uint8_t* p = reinterpret_cast<const uint8_t*>(t + i) + 16u * c;
        return FwdChunk{fwdkey_le32(p), fwdkey_le32(p + 4), fwdkey_le32(p + 8), fwdkey_le32(p + 12)};
    }
};
inline bool fwdkey_table_slots_valid(uint64_t n_slots) {
    return n_slots != 0 && (n_slots & (n_slots - 1)) == 0 && n_slots <= (1ull << 31);
}
inline bool fwdkey_lookup_host(const pipck_fwd_entry* table, uint64_t n_slots, const pipck_fwd_key& key, uint32_t& rule) {
    uint32_t k[kFwdKeyWords];
    fwdkey_words(key, k);
    return fwdkey_lookup(FwdHostTable{table}, (uint32_t)(n_slots - 1), k, fwdkey_hash(k), rule);
}

// What pipck_fwd_table_build accepts as a key: what fwdkey_parse can produce.
inline bool fwdkey_valid(const pipck_fwd_key& key) {
    if (key.pad[0] || key.pad[1]) return false;
    if (key.family != 4 && key.family != 6) return false;
    if (key.family == 4)
        for (int j = 4; j < 16; j++)
            if (key.src[j] || key.dst[j]) return false;
    const bool tcpudp = key.proto == 6 || key.proto == 17;
    if (!tcpudp && key.proto != (key.family == 4 ? 1 : 58)) return false;
    if (!tcpudp && (key.sport[0] || key.sport[1] || key.dport[0] || key.dport[1])) return false;
    return true;
}

// pipck_fwd_table_build (include/pipck.h): the table zeroed, then every key in
// order at the first empty entry of its probe sequence.
inline int fwdkey_table_build(const pipck_fwd_key* keys, const uint32_t* rules, uint64_t n_keys, pipck_fwd_entry* table,
                              uint64_t n_slots) {
    if (!table || (n_keys && (!keys || !rules)) || !fwdkey_table_slots_valid(n_slots)) return PIPCK_EINVAL;
    uint8_t* bytes = reinterpret_cast<uint8_t*>(table);
    for (uint64_t i = 0; i < n_slots * sizeof(pipck_fwd_entry); i++) bytes[i] = 0;
    const uint32_t mask = (uint32_t)(n_slots - 1);
    const FwdHostTable load{table};
    for (uint64_t n = 0; n < n_keys; n++) {
        if (!fwdkey_valid(keys[n])) return PIPCK_EINVAL;
        uint32_t k[kFwdKeyWords];
        fwdkey_words(keys[n], k);
        const uint32_t hash = fwdkey_hash(k), tag = hash | kFwdTagBit;
        uint32_t p = 0;
        for (; p < kFwdMaxProbe; p++) {
            const uint32_t i = (hash + p) & mask;
            const FwdChunk c2 = load(i, 2u);
            if (c2.w == 0u) {
                uint8_t* e = bytes + (uint64_t)i * sizeof(pipck_fwd_entry);
                for (int j = 0; j < kFwdKeyWords; j++) fwdkey_put32(e + 4 * j, k[j]);
                fwdkey_put32(e + 40, rules[n]);
                fwdkey_put32(e + 44, tag);
                break;
            }
            if (c2.w == tag && c2.x == k[8] && c2.y == k[9]) {
                const FwdChunk c0 = load(i, 0u), c1 = load(i, 1u);
                if (c0.x == k[0] && c0.y == k[1] && c0.z == k[2] && c0.w == k[3] && c1.x == k[4] && c1.y == k[5] &&
                    c1.z == k[6] && c1.w == k[7])
                    return PIPCK_EINVAL;  // a duplicate key
            }
        }
        if (p == kFwdMaxProbe) return PIPCK_ERANGE;
    }
    return PIPCK_OK;
}

}  // namespace pipck

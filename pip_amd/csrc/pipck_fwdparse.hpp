// pipck_fwdparse.hpp -- device-side parse + header rewrite of one IP frame that a
// forwarder sends on (pipck_fwd_rewrite_ring, include/pipck.h "NAT and TTL
// rewrite").  fwd_parse decides what becomes of the frame under one rule and
// computes every value to store -- the new TTL halfword, the new port word and
// both checksum fields by RFC 1624 eqn. 3 -- from the header bytes as they were
// loaded; the caller stores them afterwards, so a frame is rewritten entirely or
// not at all.  The payload is never read: an incremental update needs the old
// and the new words of the named fields and the old checksum, nothing else.
//
// The headers are walked by the rules of tx_from_window (pipck_txparse.hpp) and
// rx_from_window (pipck_rxparse.hpp).  This file calls neither and none of their
// helpers: those are plain inline functions, and a further caller changes how
// the compiler inlines them into the RX and TX kernels.  It includes
// pipck_device.hpp alone.
//
// Arithmetic.  RFC 1624 eqn. 3 in big-endian words is
//     HC' = ~fold(~HC + sum(~old_k) + sum(new_k)),
// every term a 16-bit value, the sum exact, fold the end-around carry.  fold(s)
// is 0 for s == 0 and 1 + (s - 1) mod 0xFFFF otherwise.  Swapping the bytes of
// every term multiplies the sum by 256 modulo 0xFFFF and keeps a zero sum zero
// (pipck_device.hpp), so the same sum over the halfwords as memory holds them
// (little-endian loads) folds to the byte-swapped value: all of it is done on
// the loaded dwords, dot_fold(~old, .) adding both complemented halves of a
// dword and dot_fold(new, .) both new ones, and no byte order is ever fixed.
// At most 1 + 2 * 18 terms: a u32 cannot overflow.
#pragma once
#include "pipck_device.hpp"

namespace pipck {

constexpr uint32_t kFwdSetSrc = 1, kFwdSetDst = 2, kFwdSetSport = 4, kFwdSetDport = 8, kFwdDecTtl = 16;  // PIPCK_FWD_*
constexpr uint32_t kFwdOps = 31;
constexpr uint32_t kFwdUdpZeroAsOnes = 1;                         // PIPCK_FWD_UDP_ZERO_AS_ONES
constexpr uint32_t kFwdDone = 1, kFwdExpired = 2, kFwdUnhandled = 4;  // d_done values
constexpr uint32_t kFwdNoRule = 0xFFFFFFFFu;                      // PIPCK_FWD_NO_RULE
constexpr int kFwdWords = 24;                                     // the window: 96 bytes from the frame's start

// A pipck_fwd_rule in registers, its three 16-byte chunks as loaded: addresses
// and ports are the dwords memory holds, which is how the frame's dwords hold them.
struct FwdRule {
    uint32_t ops, family;  // family: the low byte of the rule's second dword
    uint32_t src[4], dst[4];
    uint32_t ports;  // sport in the low half, dport in the high half
};
__device__ __forceinline__ FwdRule fwd_rule(const u32x4& q0, const u32x4& q1, const u32x4& q2) {
    return FwdRule{q0.x, q0.y & 0xFFu, {q0.z, q0.w, q1.x, q1.y}, {q1.z, q1.w, q2.x, q2.y}, q2.z};
}
// Unknown ops bits, a family that is none of 0, 4, 6, or family 0 with an address to set
__device__ __forceinline__ bool fwd_rule_valid(const FwdRule& r) {
    if (r.ops & ~kFwdOps) return false;
    if (r.family != 0 && r.family != 4 && r.family != 6) return false;
    return r.family != 0 || !(r.ops & (kFwdSetSrc | kFwdSetDst));
}

// What to store for one frame.  done = kFwdDone: every field of `st` is stored;
// any other done: nothing is.  Halfwords and dwords are memory's (little-endian).
constexpr uint32_t kFwdStTtl = 1, kFwdStIpSum = 2, kFwdStSrc = 4, kFwdStDst = 8, kFwdStPorts = 16, kFwdStSport = 32,
                   kFwdStDport = 64, kFwdStL4Sum = 128;
struct FwdEdit {
    uint32_t done, st;
    uint32_t v4;      // addresses: one dword at 12 / 16, else four at 8.. / 24..
    uint32_t ttl_at;  // 8 (IPv4: TTL with protocol) or 6 (IPv6: next header with hop limit)
    uint32_t ttl_hw, ip_sum;
    uint32_t l4off, ports;  // kFwdStPorts: the dword at l4off; kFwdStSport / kFwdStDport: its low / high half
    uint32_t l4_at, l4_sum;
};

// Word k (run-time) of the window; 0 past it.  A select chain: an indexed copy
// would go through scratch memory.
__device__ __forceinline__ uint32_t fwd_win_word(const uint32_t (&a)[kFwdWords], uint32_t k) {
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < kFwdWords; i++)
        if ((uint32_t)i == k) x = a[i];
    return x;
}
// Frame bytes [j, j + 4), j a multiple of 4, as memory's dword: from the window
// where it holds them all, else from the frame's own bytes one at a time (p may
// have any alignment).  The caller has bounded j + 4 by the frame's length.
__device__ __forceinline__ uint32_t fwd_word(const uint8_t* p, const uint32_t (&a)[kFwdWords], uint32_t win,
                                             uint32_t j) {
    if (j + 4u <= win) return fwd_win_word(a, j >> 2);
    return (uint32_t)p[j] | (uint32_t)p[j + 1] << 8 | (uint32_t)p[j + 2] << 16 | (uint32_t)p[j + 3] << 24;
}

// One frame under one VALID rule.  p: its first byte (any alignment); len: its
// bytes; a[k]: frame bytes [4k, 4k + 4) for 4k + 4 <= win, win >= 40 a multiple
// of 4 (a caller whose chunks are not aligned with the frame realigns them
// first, as rx_from_window does, and passes the bytes it has); words past the
// frame's end may hold anything: every range used ends at or before len.
// Reads nothing past the frame, and from memory only the extension headers and
// L4 fields of an IPv6 chain that reach past the window.
__device__ inline FwdEdit fwd_parse(const uint8_t* p, uint32_t len, const uint32_t (&a)[kFwdWords], uint32_t win,
                                    const FwdRule& r, uint32_t flags) {
    FwdEdit e{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (len < 20) return e;
    const uint32_t b0 = a[0] & 0xFFu, ver = b0 >> 4;
    const bool v4 = ver == 4;
    uint32_t ip_end, ttl, ihl = 0;
    if (v4) {
        ihl = (b0 & 15u) * 4u;
        const uint32_t total = bswap16(a[0] >> 16);
        if (ihl < 20 || total < ihl || total > len) return e;  // malformed: untouched, done 0
        ip_end = total;
        ttl = a[2] & 0xFFu;
    } else if (ver == 6 && len >= 40) {
        const uint32_t plen = bswap16(a[1] & 0xFFFFu);
        if (40 + plen > len) return e;
        ip_end = 40 + plen;
        ttl = a[1] >> 24;
    } else {
        return e;
    }
    const uint32_t ops = r.ops;
    if ((ops & kFwdDecTtl) && ttl <= 1) {  // RFC 1812 section 5.3.1: the host answers with ICMP
        e.done = kFwdExpired;
        return e;
    }
    e.done = kFwdUnhandled;
    if (r.family != 0 && r.family != ver) return e;
    const bool addr = ops & (kFwdSetSrc | kFwdSetDst), port = ops & (kFwdSetSport | kFwdSetDport);
    uint32_t proto = 0, l4off = 0;
    if (addr || port) {  // a rule with DEC_TTL alone never looks at the upper layer
        if (v4) {
            if (bswap16(a[1] >> 16) & 0x3FFFu) return e;  // a fragment
            proto = (a[2] >> 8) & 0xFFu;
            l4off = ihl;
        } else {
            // hop-by-hop 0, destination options 60 and atomic fragments 44 are walked, at most 8 of them
            uint32_t nh = a[1] >> 16 & 0xFFu, at = 40;
            bool up = false;
            for (int k = 0; k < 9; k++) {
                if (nh != 0 && nh != 60 && nh != 44) {
                    up = nh != 43;  // a routing header
                    break;
                }
                if (k == 8) break;           // a ninth extension header
                if (at + 8 > ip_end) break;  // does not fit in the payload
                const uint32_t x = fwd_word(p, a, win, at);  // next header, length, and a fragment's field
                if (nh == 44) {
                    if (bswap16(x >> 16) & 0xFFF9u) break;  // an offset or M
                    at += 8;
                } else {
                    at += 8u * ((x >> 8 & 0xFFu) + 1u);
                }
                if (at > ip_end) break;
                nh = x & 0xFFu;
            }
            if (!up) return e;
            proto = nh;
            l4off = at;
        }
        const bool tcpudp = proto == 6u || proto == 17u;
        if (port && !tcpudp) return e;
        if (!tcpudp && proto != (v4 ? 1u : 58u)) return e;
        if (ip_end - l4off < (proto == 6u ? 20u : 8u)) return e;  // no room for the L4 fields
    }

    // DONE: every value from the bytes as loaded
    e.v4 = v4;
    uint32_t sip = 0, sl4 = 0;  // sum(~old) + sum(new) of the named words each field covers
    if (ops & kFwdDecTtl) {
        e.st |= kFwdStTtl;
        if (v4) {  // bytes 8-9: TTL, protocol
            const uint32_t old = a[2] & 0xFFFFu;
            e.ttl_at = 8, e.ttl_hw = old - 1u;  // TTL >= 2: no borrow
            sip += (0xFFFFu - old) + e.ttl_hw;
        } else {  // bytes 6-7: next header, hop limit; no header checksum
            e.ttl_at = 6, e.ttl_hw = (a[1] >> 16) - 0x100u;
        }
    }
    uint32_t sad = 0;  // the address words: the IPv4 header field and, through the pseudo-header, the L4 field
    if (ops & kFwdSetSrc) {
        e.st |= kFwdStSrc;
        if (v4) {
            sad = dot_fold(r.src[0], dot_fold(~a[3], sad));
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) sad = dot_fold(r.src[k], dot_fold(~a[2 + k], sad));
        }
    }
    if (ops & kFwdSetDst) {
        e.st |= kFwdStDst;
        if (v4) {
            sad = dot_fold(r.dst[0], dot_fold(~a[4], sad));
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) sad = dot_fold(r.dst[k], dot_fold(~a[6 + k], sad));
        }
    }
    sip += sad;
    if (v4 && (ops & (kFwdDecTtl | kFwdSetSrc | kFwdSetDst))) {
        e.st |= kFwdStIpSum;
        e.ip_sum = 0xFFFFu - fold16((0xFFFFu - (a[2] >> 16)) + sip);
    }
    if (addr || port) {
        const bool icmp4 = v4 && proto == 1u;
        if (!icmp4) sl4 = sad;  // ICMP over IPv4 has no pseudo-header
        if (port) {
            const uint32_t old = fwd_word(p, a, win, l4off);
            const uint32_t m = ((ops & kFwdSetSport) ? 0xFFFFu : 0u) | ((ops & kFwdSetDport) ? 0xFFFF0000u : 0u);
            e.l4off = l4off;
            e.ports = (old & ~m) | (r.ports & m);
            e.st |= m == 0xFFFFFFFFu ? kFwdStPorts : (ops & kFwdSetSport) ? kFwdStSport : kFwdStDport;
            sl4 = dot_fold(r.ports & m, dot_fold(~old & m, sl4));
        }
        if (!icmp4) {  // else the field's word list is empty (a port rule needs TCP or UDP): not touched
            const uint32_t at = l4off + (proto == 6u ? 16u : proto == 17u ? 6u : 2u);
            const uint32_t old = fwd_word(p, a, win, at & ~3u) >> (8u * (at & 2u)) & 0xFFFFu;
            if (!(proto == 17u && v4 && old == 0u)) {  // RFC 3022 section 4.1: no checksum was sent, none is
                uint32_t val = 0xFFFFu - fold16((0xFFFFu - old) + sl4);
                if (proto == 17u && val == 0u && (flags & kFwdUdpZeroAsOnes)) val = 0xFFFFu;
                e.st |= kFwdStL4Sum;
                e.l4_at = at;
                e.l4_sum = val;
            }
        }
    }
    e.done = kFwdDone;
    return e;
}

}  // namespace pipck

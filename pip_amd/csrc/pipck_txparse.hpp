// pipck_txparse.hpp -- device-side parse + checksum fill of one IP frame about
// to be sent (pipck_tx_fill_device, include/pipck.h "TX checksum fill").  The TX
// mirror of pipck_rxparse.hpp: k_packedb_tx (pipck_packedb.hip) calls
// tx_from_window at each tile's end with the frame sum it has just streamed and
// the header window it captured -- as k_ring_tx (pipck_txring.hip) does at each
// block's end for frames in ring slots -- and stores the two fields this returns: the
// bytes pip's TX path writes (th_sum, pip/protocol/pip_tcp_packet.cpp:124-134;
// uh_sum, pip/protocol/pip_udp.cpp:40-61; ip_sum, pip/pip_netif.cpp:80-97).
//
// tx_from_window stands beside rx_from_window (the yardstick of the RX tests,
// left as it is) and walks the headers by the same rules; it uses that file's
// window helpers.
//
// Arithmetic.  Everything comes from the one streamed frame sum sall, as on RX:
// the L4 range is the frame minus what precedes it (pre), minus the link padding
// (post), minus the checksum field as it was loaded (old), plus the
// pseudo-header,
//     x = sall + (0xFFFF - pre) + (0xFFFF - post) + (0xFFFF - old) + pseudo.
// Every term is non-negative and x > 0, so fold16(x) lies in 1..0xFFFF and equals
// pip's fold of the true sum T (pip_checksum.cpp:29-30) whenever T > 0; the value
// stored is its complement, 0x0000 included (a computed zero stays zero,
// include/pipck.h).  T == 0 is possible for an all-zero ICMPv4 message only --
// the pseudo-header's protocol + length and the IPv4 version nibble keep every
// other range non-zero -- and is decided, as rx_from_window decides it, by
// looking at the message's bytes: pip's ~fold(0) = 0xFFFF.  Subtracting the old
// field is what makes "the field taken as zero" hold whatever the field held, so
// filling twice gives the same bytes.
#pragma once
#include "pipck_rxparse.hpp"

namespace pipck {

constexpr uint32_t kTxIp = 1, kTxL4 = 2;  // PIPCK_TX_IP_FILLED / PIPCK_TX_L4_FILLED (include/pipck.h)
constexpr uint32_t kTxUdpZeroAsOnes = 1;  // PIPCK_TX_UDP_ZERO_AS_ONES

// What to store for one frame: done = the PIPCK_TX_* bits; with kTxIp, ip_val
// goes big-endian to frame bytes 10-11; with kTxL4, l4_val to bytes l4_at and
// l4_at + 1.  Nothing has been stored yet: the caller stores once both values
// are known, so each is computed from the bytes as they were loaded.
struct TxFill {
    uint32_t done, ip_val, l4_at, l4_val;
};

// Frame bytes [lo, hi) read from memory one byte at a time, as mem_sum / mem_any /
// range_sum of pipck_rxparse.hpp.  Copies of this file's own: those are plain
// inline functions with k_packedb_rx as their one caller, and a second caller
// would change how the compiler inlines them there -- the RX kernel's code stays
// exactly what it was.
__device__ inline uint32_t tx_mem_sum(const uint8_t* p, uint32_t lo, uint32_t hi) {
    uint32_t s = 0;
    for (uint32_t j = lo; j < hi; j++) s += (uint32_t)p[j] << (8u * (j & 1u));
    return fold16(s);
}
__device__ inline bool tx_mem_any(const uint8_t* p, uint32_t lo, uint32_t hi) {
    for (uint32_t j = lo; j < hi; j++)
        if (p[j]) return true;
    return false;
}
__device__ __forceinline__ uint32_t tx_range_sum(const uint8_t* p, const uint32_t (&a)[kWinWords], uint32_t lo,
                                                 uint32_t hi) {
    uint32_t s = lo < 4u * kWinWords ? win_sum(a, lo, min(hi, 4u * kWinWords)) : 0u;
    if (hi > 4u * kWinWords) s += tx_mem_sum(p, max(lo, 4u * kWinWords), hi);
    return s;
}

// One frame: p its first byte (any alignment), len its bytes, sall the folded
// big-endian sum of the whole frame from the stream, w its header window
// (rx_window_global's chunks), flags the call's PIPCK_TX_* flags.  Reads nothing
// past the frame; fields and ranges past the 80-byte window (long IPv6 extension
// chains, long link padding) are read from the frame's bytes in memory.
__device__ inline TxFill tx_from_window(const uint8_t* p, uint32_t len, uint32_t sall, const uint32_t (&w)[24],
                                        uint32_t flags) {
    TxFill out{0u, 0u, 0u, 0u};
    if (len < 20) return out;
    const uint32_t h = (uint32_t)((uintptr_t)p & 15u);
    // realign: a[k] = bytes [4k, 4k + 4) of the frame (masked blends, as rx_from_window)
    const uint32_t q = h >> 2, r = h & 3u;
    const uint32_t m2 = 0u - ((q >> 1) & 1u), m1 = 0u - (q & 1u);
    uint32_t u[23], a[kWinWords];
#pragma unroll
    for (int k = 0; k < 22; k++) u[k] = w[k] ^ ((w[k] ^ w[k + 2]) & m2);
    u[22] = w[22] & ~m2;
#pragma unroll
    for (int k = 0; k < 21; k++) u[k] = u[k] ^ ((u[k] ^ u[k + 1]) & m1);
#pragma unroll
    for (int k = 0; k < kWinWords; k++) a[k] = __builtin_amdgcn_alignbyte(u[k + 1], u[k], r);

    const uint32_t b0 = a[0] & 0xFFu;
    uint32_t ip_end, l4off, proto;
    uint32_t le_pre;  // LE sum of [0, l4off), bytes as loaded
    uint32_t pseudo_addr;
    const bool v4 = (b0 >> 4) == 4;
    if (v4) {
        const uint32_t ihl = (b0 & 15u) * 4u, total = win_be16(a, 2);
        if (ihl < 20 || total < ihl || total > len) return out;  // malformed: not written
        uint32_t hs = 0;  // the whole header, exactly (<= 60 bytes: inside the window)
#pragma unroll
        for (int k = 0; k < 15; k++)
            if ((uint32_t)k < ihl / 4u) hs = dot_fold(a[k], hs);
        // bytes 10-11 are the high half of a[2], one LE word of hs: hs - old is the
        // exact LE sum of the header with the field zeroed, and > 0 (the version nibble)
        const uint32_t old_ip = a[2] >> 16;
        out.ip_val = 0xFFFFu - bswap16(fold16(hs - old_ip));
        out.done = kTxIp;
        if (win_be16(a, 6) & 0x3FFFu) return out;  // a fragment: the header field only
        proto = win_byte(a, 9);
        l4off = ihl;
        ip_end = total;
        le_pre = hs;
        pseudo_addr = bswap16(fold16(dot_fold(a[3], dot_fold(a[4], 0u))));  // [12, 20)
    } else if ((b0 >> 4) == 6 && len >= 40) {
        const uint32_t plen = win_be16(a, 4);
        if (40 + plen > len) return out;
        ip_end = 40 + plen;
        // the upper-layer header, located as rx_from_window locates it: hop-by-hop 0,
        // destination options 60 and atomic fragments 44 are walked, at most 8 of them
        uint32_t nh = win_byte(a, 6), at = 40;
        bool up = false;
        for (int k = 0; k < 9; k++) {
            if (nh != 0 && nh != 60 && nh != 44) {
                up = nh != 43;  // a routing header: nothing written
                break;
            }
            if (k == 8) break;            // a ninth extension header
            if (at + 8 > ip_end) break;   // does not fit in the payload
            const uint32_t next = mem_byte(p, a, at);
            if (nh == 44) {
                if (((mem_byte(p, a, at + 2) << 8) | mem_byte(p, a, at + 3)) & 0xFFF9u) break;  // an offset or M
                at += 8;
            } else {
                at += 8u * (mem_byte(p, a, at + 1) + 1u);
            }
            if (at > ip_end) break;
            nh = next;
        }
        if (!up) return out;
        proto = nh;
        l4off = at;
        if (l4off == 40) {  // no extension headers (the common case): the fixed header's ten words
            uint32_t f = 0;
#pragma unroll
            for (int k = 0; k < 10; k++) f = dot_fold(a[k], f);
            le_pre = f;
        } else {
            le_pre = tx_range_sum(p, a, 0, l4off);
        }
        uint32_t s = 0;
#pragma unroll
        for (int k = 2; k < 10; k++) s = dot_fold(a[k], s);  // [8, 40)
        pseudo_addr = bswap16(fold16(s));
    } else {
        return out;
    }
    const bool icmp4 = v4 && proto == 1u;
    if (proto != 6u && proto != 17u && !icmp4 && !(!v4 && proto == 58u)) return out;  // no checksum this knows
    const uint32_t l4len = ip_end - l4off;
    if (l4len < (proto == 6u ? 20u : 8u)) return out;  // truncated: no L4 field
    // the field: message offset 16 (TCP), 6 (UDP), 2 (ICMP, ICMPv6); l4off is a
    // multiple of 4, so it is one big-endian word of the frame's sum
    const uint32_t at = l4off + (proto == 6u ? 16u : proto == 17u ? 6u : 2u);
    const uint32_t old = (mem_byte(p, a, at) << 8) | mem_byte(p, a, at + 1);
    const uint32_t pre = bswap16(fold16(le_pre));
    const uint32_t post = ip_end < len ? bswap16(fold16(tx_range_sum(p, a, ip_end, len))) : 0u;
    const uint32_t P = icmp4 ? 0u : proto + pseudo_addr + (l4len >> 16) + (l4len & 0xFFFFu);
    const uint32_t x = sall + (0xFFFFu - pre) + (0xFFFFu - post) + (0xFFFFu - old) + P;
    uint32_t val = 0xFFFFu - fold16(x);
    if (icmp4 && val == 0u) {  // sum == 0 (mod 0xFFFF): an all-zero message (field apart) sums to 0, not 0xFFFF
        const bool nonzero = win_sum(a, l4off, l4off + 2) != 0 || win_sum(a, l4off + 4, l4off + 8) != 0 ||
                             tx_mem_any(p, l4off + 8, ip_end);
        if (!nonzero) val = 0xFFFFu;  // pip's ~fold(0)
    }
    if (proto == 17u && val == 0u && (flags & kTxUdpZeroAsOnes)) val = 0xFFFFu;  // RFC 768, RFC 8200 section 8.1
    out.done |= kTxL4;
    out.l4_at = at;
    out.l4_val = val;
    return out;
}

}  // namespace pipck

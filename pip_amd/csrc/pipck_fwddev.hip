// pipck_fwddev.hip -- NAT and TTL rewrite of IP frames in a byte-packed batch in
// device memory (pipck_fwd_rewrite_device, include/pipck.h): the frames back to
// back at any byte offset, found through the tile index of
// pipck_packed_bytes_index, rewritten from their headers alone by the rules and
// the arithmetic of pipck_fwd_rewrite_ring (fwd_parse, pipck_fwdparse.hpp).  The
// payload is never read, so the traffic is set by header lines, not frame bytes.
//
// A file of its own: it includes the forwarding parse and nothing of the RX and
// TX parse headers, so every other kernel of the library compiles to exactly the
// code it had.
#include "pipck_common.hpp"
#include "pipck_fwdparse.hpp"

namespace pipck {

constexpr uint32_t kFwdDevB = 256;  // frames per block: one tile of 64 per wave, the four waves independent
static_assert(sizeof(pipck_fwd_rule) == 48 && alignof(pipck_fwd_rule) <= 16, "pipck_fwd_rule is three 16-byte chunks");
static_assert(kFwdSetSrc == PIPCK_FWD_SET_SRC && kFwdSetDst == PIPCK_FWD_SET_DST &&
                  kFwdSetSport == PIPCK_FWD_SET_SPORT && kFwdSetDport == PIPCK_FWD_SET_DPORT &&
                  kFwdDecTtl == PIPCK_FWD_DEC_TTL && kFwdUdpZeroAsOnes == PIPCK_FWD_UDP_ZERO_AS_ONES &&
                  kFwdDone == PIPCK_FWD_DONE && kFwdExpired == PIPCK_FWD_EXPIRED &&
                  kFwdUnhandled == PIPCK_FWD_UNHANDLED && kFwdNoRule == PIPCK_FWD_NO_RULE,
              "pipck_fwdparse.hpp restates include/pipck.h");

// Field stores.  A field's offset in its frame is even, and that of an address,
// a port pair or l4off a multiple of 4, so the widest store that covers bytes of
// this frame alone follows from the frame's absolute start, al = start & 3:
// al == 0 the ring kernel's aligned dwords and halfwords, al == 2 halfwords,
// odd single bytes.  None is a read-modify-write of a wider unit, so the bytes
// of the neighbouring frame in the same dword may be stored by another lane,
// wave or block at the same time.  v: memory's little-endian value.  Default
// cache policy (store_field8), range-checked against the tile's own bytes.
__device__ __forceinline__ void put_field16(buf_t r, uint32_t off, uint32_t v, uint32_t al) {
    if (al & 1u) {
        store_field8(r, off, v & 0xFFu);
        store_field8(r, off + 1u, v >> 8 & 0xFFu);
    } else {
        store_field16(r, off, v);
    }
}
__device__ __forceinline__ void put_field32(buf_t r, uint32_t off, uint32_t v, uint32_t al) {
    if (al == 0u) {
        __builtin_amdgcn_raw_buffer_store_b32(v, r, (int)off, 0, 0);
    } else {
        put_field16(r, off, v & 0xFFFFu, al);
        put_field16(r, off + 2u, v >> 16, al);
    }
}

// A wave takes one tile of 64 frames, lane g frame g: its length, its start (the
// tile's offset plus the exclusive scan of the lengths), its rule index.  The
// tile bound comes first, scalar and overflow-safe as in packedb_body: a tile
// whose bytes reach past arena_bytes is neither read nor written, its frames
// get done 0 and err PIPCK_ERANGE, and its rules are not looked at.  Then per
// frame the refusal of an index past the table, and Lw = min(length, 96), 0 for
// a refused frame, a frame without a rule and a lane past the batch: such a
// frame is neither read nor written.
//
// The window loads keep k_fwd_ring's scheme: eight lanes per frame, lane 8j + c
// loading aligned chunk c of frame 8k + j, so one instruction reads eight
// windows.  A frame starts h = start & 15 bytes into its first chunk; SIX chunks
// are loaded, chunk c iff 16 c < h + Lw (never one past the chunk holding the
// frame's last byte), and fwd_parse is told win = (96 - h) & ~3, the bytes the
// six chunks are sure to hold (80 at least; IPv4 needs 78).  Past win it reads
// the frame's own bytes, as it does for a long IPv6 extension chain.  The loads
// go through a resource that ends with the chunk holding the tile's last byte.
// Bytes of other frames that share a chunk -- they may be rewritten by another
// lane, wave or block meanwhile -- are shifted out by the realignment or lie
// past the frame's length, where fwd_parse uses nothing: no result depends on
// whether such a load saw the old or the new bytes.
//
// The chunks go through the wave's own 6 x 65 x 16 bytes of LDS and come back
// as 24 dwords in the frame's lane (no block barrier: a wave reads only what it
// wrote), which realigns them as rx_from_window does: masked blends by 2 and 1
// dwords, then v_alignbyte by h & 3 -- static register indices throughout.
//
// fwd_parse gives every value, then the lane stores them (put_field16/32)
// through a resource that ends with the tile's last frame byte.  Every store
// lies inside the lane's own frame: fwd_parse names only fields it has bounded
// by the IP length.
__global__ __launch_bounds__(256) void k_fwd_device(uint8_t* arena, uint64_t arena_bytes,
                                                    const uint16_t* __restrict__ lens,
                                                    const uint64_t* __restrict__ tile_off, uint64_t n,
                                                    const u32x4* __restrict__ rules, uint32_t n_rules,
                                                    const uint32_t* __restrict__ rule_of, uint32_t flags,
                                                    uint8_t* __restrict__ done, uint32_t* __restrict__ err) {
    __shared__ u32x4 hdr[kFwdDevB / 64][6][65];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t tile = (uint64_t)blockIdx.x * (kFwdDevB / 64) + w;
    const uint64_t s0 = tile * 64;  // the wave's first frame
    if (s0 >= n) return;
    const uint32_t nw = (uint32_t)min<uint64_t>(64, n - s0);
    const bool valid = lane < nw;
    const uint32_t L = valid ? (uint32_t)lens[s0 + lane] : 0u;
    const uint32_t ri = !valid ? kFwdNoRule : rule_of ? rule_of[s0 + lane] : 0u;
    const buf_t db = buf_rsrc(done + s0, nw);

    const uint32_t incl = wave_incl_scan(L);
    const uint64_t toff = first_lane_u64(tile_off[tile]);
    const uint32_t tile_len = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (!(toff <= arena_bytes && (uint64_t)tile_len <= arena_bytes - toff)) {  // wave-uniform
        refuse(err, lane == 0);
        store_result8(db, lane, 0u);
        return;
    }
    const uint64_t first = (uint64_t)(uintptr_t)arena + toff;
    const uint64_t base = first & ~15ull;  // the chunk holding the tile's first byte
    const uint32_t lead = (uint32_t)(first - base);
    const uint32_t start = lead + incl - L;  // relative to base
    const uint32_t h = start & 15u;

    const bool bad = valid && ri != kFwdNoRule && ri >= n_rules;  // bounded before the table is read
    const bool go = valid && !bad && ri != kFwdNoRule;
    const uint32_t Lw = go ? min(L, 4u * kFwdWords) : 0u;

    u32x4 q0{0u, 0u, 0u, 0u}, q1 = q0, q2 = q0;
    if (go) {
        const u32x4* rp = rules + 3ull * ri;
        q0 = load_plain(rp), q1 = load_plain(rp + 1), q2 = load_plain(rp + 2);
    }

    const buf_t lb = buf_rsrc(reinterpret_cast<const void*>(base), (lead + tile_len + 15u) & ~15u);  // whole chunks
    const uint32_t c = lane & 7u, sub = lane >> 3;
    const uint32_t mine = start << 7 | Lw;  // start < 2^23, Lw <= 96
    u32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t s = 8u * k + sub;
        const uint32_t x = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4u * s), (int)mine);
        const uint32_t ss = x >> 7, Ls = x & 127u;
        v[k] = Ls != 0u && 16u * c < (ss & 15u) + Ls && c < 6u ? buf_load<false>(lb, (ss & ~15u) + 16u * c)
                                                                 : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (c < 6u) hdr[w][c][8u * k + sub] = v[k];
    wave_sync();
    // realign: a[k] = frame bytes [4k, 4k + 4) for 4k + 4 <= win
    const uint32_t q = h >> 2, r8 = h & 3u;
    const uint32_t m2 = 0u - ((q >> 1) & 1u), m1 = 0u - (q & 1u);
    uint32_t u[kFwdWords + 3], a[kFwdWords];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const u32x4 x = hdr[w][k][lane];
        u[4 * k] = x.x, u[4 * k + 1] = x.y, u[4 * k + 2] = x.z, u[4 * k + 3] = x.w;
    }
    u[24] = u[25] = u[26] = 0u;
#pragma unroll
    for (int k = 0; k < kFwdWords + 1; k++) u[k] = u[k] ^ ((u[k] ^ u[k + 2]) & m2);
#pragma unroll
    for (int k = 0; k < kFwdWords + 1; k++) u[k] = u[k] ^ ((u[k] ^ u[k + 1]) & m1);
#pragma unroll
    for (int k = 0; k < kFwdWords; k++) a[k] = __builtin_amdgcn_alignbyte(u[k + 1], u[k], r8);

    const FwdRule r = fwd_rule(q0, q1, q2);
    const bool inv = go && !fwd_rule_valid(r);  // the frame untouched, done 0, PIPCK_EINVAL
    FwdEdit e{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (go && !inv)
        e = fwd_parse(reinterpret_cast<const uint8_t*>(base) + start, L, a, (4u * kFwdWords - h) & ~3u, r, flags);

    // every value is known: memory gets them
    const buf_t wb = buf_rsrc(reinterpret_cast<const void*>(base), lead + tile_len);  // ends with the last frame
    const uint32_t at = start, al = start & 3u;
    const uint32_t st = e.done == kFwdDone ? e.st : 0u;
    if (st & kFwdStTtl) put_field16(wb, at + e.ttl_at, e.ttl_hw, al);
    if (st & kFwdStIpSum) put_field16(wb, at + 10u, e.ip_sum, al);
    if (st & kFwdStSrc) {
        if (e.v4) {
            put_field32(wb, at + 12u, r.src[0], al);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) put_field32(wb, at + 8u + 4u * k, r.src[k], al);
        }
    }
    if (st & kFwdStDst) {
        if (e.v4) {
            put_field32(wb, at + 16u, r.dst[0], al);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) put_field32(wb, at + 24u + 4u * k, r.dst[k], al);
        }
    }
    if (st & kFwdStPorts) put_field32(wb, at + e.l4off, e.ports, al);
    if (st & kFwdStSport) put_field16(wb, at + e.l4off, e.ports & 0xFFFFu, al);
    if (st & kFwdStDport) put_field16(wb, at + e.l4off + 2u, e.ports >> 16, al);
    if (st & kFwdStL4Sum) put_field16(wb, at + e.l4_at, e.l4_sum, al);
    refuse(err, bad);
    if (inv && err) atomicOr(err, 1u << PIPCK_EINVAL);
    store_result8(db, lane, e.done);
}

// pipck_fwd_rewrite_device: the byte-packed calls' argument rules plus the rule
// table's, then one k_fwd_device over blocks of four tiles -- nothing allocated,
// nothing remembered, so the call can be captured
static int launch_packedb_fwd(void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens, const uint64_t* d_tile_off,
                              uint64_t n, const pipck_fwd_rule* d_rules, uint32_t n_rules, const uint32_t* d_rule_of,
                              uint32_t flags, uint8_t* d_done, uint32_t* d_err, hipStream_t s) {
    if (flags & ~(uint32_t)PIPCK_FWD_UDP_ZERO_AS_ONES) {
        set_error("pipck_fwd_rewrite_device: unknown flag bits");
        return PIPCK_EINVAL;
    }
    if (n == 0) return PIPCK_OK;
    if (!d_arena || !d_lens || !d_tile_off || !d_done || !d_rules) {
        set_error("pipck_fwd_rewrite_device: null pointer");
        return PIPCK_EINVAL;
    }
    if (n_rules == 0 || (uintptr_t)d_rules % 16) {
        set_error("pipck_fwd_rewrite_device: the rule table must be 16-byte aligned and hold at least one rule");
        return PIPCK_EINVAL;
    }
    if ((uintptr_t)d_arena % 128) {
        set_error("pipck_fwd_rewrite_device: the arena must be 128-byte aligned");
        return PIPCK_EINVAL;
    }
    const uint64_t tiles = (n + 63) / 64;
    if (tiles > 0x7FFFFFFFull) {
        set_error("pipck_fwd_rewrite_device: more than 2^37 packets in one launch");
        return PIPCK_ERANGE;
    }
    const uint64_t blocks = (tiles + kFwdDevB / 64 - 1) / (kFwdDevB / 64);
    PIPCK_LAUNCH(k_fwd_device, dim3((uint32_t)blocks), dim3(256), 0, s, (uint8_t*)d_arena, arena_bytes, d_lens,
                 d_tile_off, n, (const u32x4*)d_rules, n_rules, d_rule_of, flags, d_done, d_err);
    PIPCK_LAUNCHED("k_fwd_device");
    return PIPCK_OK;
}

}  // namespace pipck

extern "C" {

int pipck_fwd_rewrite_device(void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens, const uint64_t* d_tile_off,
                             uint64_t n_packets, const pipck_fwd_rule* d_rules, uint32_t n_rules,
                             const uint32_t* d_rule_of, uint32_t flags, uint8_t* d_done, uint32_t* d_err, void* stream) {
    return pipck::launch_packedb_fwd(d_arena, arena_bytes, d_lens, d_tile_off, n_packets, d_rules, n_rules, d_rule_of,
                                     flags, d_done, d_err, pipck::as_stream(stream));
}

}  // extern "C"

// pipck_fwd.hip -- NAT and TTL rewrite of IP frames in the fixed-size slots of a
// ring in device memory (pipck_fwd_rewrite_ring, include/pipck.h), from the
// headers alone: per frame the kernel loads the first 96 bytes, changes the
// fields its rule names and updates the IPv4 header and L4 checksum fields by
// RFC 1624 eqn. 3 (fwd_parse, pipck_fwdparse.hpp).  The payload is never read,
// so the traffic is set by header lines -- one per frame, two where the fields
// straddle byte 128 of the slot -- and not by frame bytes.
//
// A file of its own, with a parse of its own (see pipck_fwdparse.hpp): every
// other kernel of the library compiles to exactly the code it had.
#include "pipck_common.hpp"
#include "pipck_fwdparse.hpp"

namespace pipck {

constexpr uint32_t kFwdB = 256;  // slots per block: 64 per wave, the four waves independent of each other
static_assert(sizeof(pipck_fwd_rule) == 48 && alignof(pipck_fwd_rule) <= 16, "pipck_fwd_rule is three 16-byte chunks");
static_assert(kFwdSetSrc == PIPCK_FWD_SET_SRC && kFwdSetDst == PIPCK_FWD_SET_DST &&
                  kFwdSetSport == PIPCK_FWD_SET_SPORT && kFwdSetDport == PIPCK_FWD_SET_DPORT &&
                  kFwdDecTtl == PIPCK_FWD_DEC_TTL && kFwdUdpZeroAsOnes == PIPCK_FWD_UDP_ZERO_AS_ONES &&
                  kFwdDone == PIPCK_FWD_DONE && kFwdExpired == PIPCK_FWD_EXPIRED &&
                  kFwdUnhandled == PIPCK_FWD_UNHANDLED && kFwdNoRule == PIPCK_FWD_NO_RULE,
              "pipck_fwdparse.hpp restates include/pipck.h");

// Address and port stores: one aligned dword each (offsets 12 and 16, 8..36 and
// l4off are multiples of 4 in a slot that starts at a multiple of 16), with the
// default cache policy of store_field16, so the L2 merges a frame's stores into
// the line the window load has just brought in.
__device__ __forceinline__ void store_field32(buf_t r, uint32_t byte_off, uint32_t v) {
    __builtin_amdgcn_raw_buffer_store_b32(v, r, (int)byte_off, 0, 0);
}

// A wave takes 64 slots, lane g slot g: its length, its rule index, the refusals
// (a length past the stride, an index past the table) and the window bytes the
// slot may load, Lw = min(length, 96) -- 0 for a refused slot, a slot without a
// rule and a lane past the ring's end: such a slot is neither read nor written.
//
// The window loads.  One lane per slot walking its six chunks would make every
// load instruction touch 64 lines for 16 bytes each.  Instead eight lanes take
// one slot, lane 8j + c chunk c (c < 6; two lanes idle), so one instruction
// reads the contiguous windows of eight slots, and eight instructions, all in
// flight together, those of the wave's 64.  Chunk c is loaded iff 16 c < Lw of
// its slot (ds_bpermute hands the lengths over); the others are zeros.  The
// chunks go through the wave's own 6 x 65 x 16 bytes of LDS (65: the eight
// lanes of a slot write to banks 4 dwords apart, not to one) and come back as
// 24 dwords in the slot's lane.  No block barrier: a wave reads only what it
// wrote.
//
// The rule is gathered by index, three 16-byte loads from a small cached table,
// only for an index inside it.  fwd_parse then gives every value from the bytes
// as loaded, and the lane stores them: aligned halfwords for the TTL and the
// checksum fields, dwords for addresses and a port pair.  Every store lies
// inside the frame (fwd_parse names only fields it has bounded by the IP
// length), hence inside the slot and inside the resource of the wave's slots.
// Far fields -- an IPv6 extension chain that carries the L4 header past byte 96
// -- are read by fwd_parse from the frame's own bytes.
__global__ __launch_bounds__(256) void k_fwd_ring(uint8_t* arena, uint32_t stride, const uint16_t* __restrict__ lens,
                                                  uint64_t n, const u32x4* __restrict__ rules, uint32_t n_rules,
                                                  const uint32_t* __restrict__ rule_of, uint32_t flags,
                                                  uint8_t* __restrict__ done, uint32_t* __restrict__ err) {
    __shared__ u32x4 hdr[kFwdB / 64][6][65];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t s0 = (uint64_t)blockIdx.x * kFwdB + 64u * w;  // the wave's first slot
    if (s0 >= n) return;
    const uint32_t nw = (uint32_t)min<uint64_t>(64, n - s0);
    const bool valid = lane < nw;
    const uint32_t L = valid ? (uint32_t)lens[s0 + lane] : 0u;
    const uint32_t ri = !valid ? kFwdNoRule : rule_of ? rule_of[s0 + lane] : 0u;
    const bool bad = valid && (L > stride || (ri != kFwdNoRule && ri >= n_rules));  // bounded before any access
    const bool go = valid && !bad && ri != kFwdNoRule;
    const uint32_t Lw = go ? min(L, 4u * kFwdWords) : 0u;

    u32x4 q0{0u, 0u, 0u, 0u}, q1 = q0, q2 = q0;
    if (go) {
        const u32x4* rp = rules + 3ull * ri;
        q0 = load_plain(rp), q1 = load_plain(rp + 1), q2 = load_plain(rp + 2);
    }

    const buf_t rb = buf_rsrc(arena + s0 * stride, nw * stride);  // the wave's slots: its loads and its stores
    const uint32_t c = lane & 7u, sub = lane >> 3;
    u32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t s = 8u * k + sub;
        const uint32_t Ls = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(4u * s), (int)Lw);
        v[k] = 16u * c < Ls && c < 6u ? buf_load<false>(rb, s * stride + 16u * c) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (c < 6u) hdr[w][c][8u * k + sub] = v[k];
    wave_sync();
    uint32_t a[kFwdWords];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const u32x4 x = hdr[w][k][lane];
        a[4 * k] = x.x, a[4 * k + 1] = x.y, a[4 * k + 2] = x.z, a[4 * k + 3] = x.w;
    }

    const FwdRule r = fwd_rule(q0, q1, q2);
    const bool inv = go && !fwd_rule_valid(r);  // the frame untouched, done 0, PIPCK_EINVAL
    FwdEdit e{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (go && !inv) e = fwd_parse(arena + (s0 + lane) * stride, L, a, 4u * kFwdWords, r, flags);

    // every value is known: memory gets them
    const uint32_t at = lane * stride;
    const uint32_t st = e.done == kFwdDone ? e.st : 0u;
    if (st & kFwdStTtl) store_field16(rb, at + e.ttl_at, e.ttl_hw);
    if (st & kFwdStIpSum) store_field16(rb, at + 10u, e.ip_sum);
    if (st & kFwdStSrc) {
        if (e.v4) {
            store_field32(rb, at + 12u, r.src[0]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) store_field32(rb, at + 8u + 4u * k, r.src[k]);
        }
    }
    if (st & kFwdStDst) {
        if (e.v4) {
            store_field32(rb, at + 16u, r.dst[0]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) store_field32(rb, at + 24u + 4u * k, r.dst[k]);
        }
    }
    if (st & kFwdStPorts) store_field32(rb, at + e.l4off, e.ports);
    if (st & kFwdStSport) store_field16(rb, at + e.l4off, e.ports);
    if (st & kFwdStDport) store_field16(rb, at + e.l4off + 2u, e.ports >> 16);
    if (st & kFwdStL4Sum) store_field16(rb, at + e.l4_at, e.l4_sum);
    refuse(err, bad);
    if (inv && err) atomicOr(err, 1u << PIPCK_EINVAL);
    store_result8(buf_rsrc(done + s0, nw), lane, e.done);
}

// pipck_fwd_rewrite_ring: pipck_tx_fill_ring's argument rules plus the rule
// table's, then one k_fwd_ring over blocks of 256 slots -- nothing allocated,
// no ring remembered, so the call can be captured
int launch_ring_fwd(void* d_arena, uint64_t stride, const uint16_t* d_lens, uint64_t n, const pipck_fwd_rule* d_rules,
                    uint32_t n_rules, const uint32_t* d_rule_of, uint32_t flags, uint8_t* d_done, uint32_t* d_err,
                    hipStream_t s) {
    if (flags & ~(uint32_t)PIPCK_FWD_UDP_ZERO_AS_ONES) {
        set_error("pipck_fwd_rewrite_ring: unknown flag bits");
        return PIPCK_EINVAL;
    }
    if (n == 0) return PIPCK_OK;
    if (!d_arena || !d_lens || !d_done || !d_rules) {
        set_error("pipck_fwd_rewrite_ring: null pointer");
        return PIPCK_EINVAL;
    }
    if (n_rules == 0 || (uintptr_t)d_rules % 16) {
        set_error("pipck_fwd_rewrite_ring: the rule table must be 16-byte aligned and hold at least one rule");
        return PIPCK_EINVAL;
    }
    if ((uintptr_t)d_arena % 16 || stride % 16 || stride < 1024 || stride > 65536) {
        set_error("pipck_fwd_rewrite_ring: the arena must be 16-byte aligned and the slot stride a multiple of 16 "
                  "bytes from 1 KiB to 64 KiB");
        return PIPCK_EINVAL;
    }
    const uint64_t blocks = (n + kFwdB - 1) / kFwdB;
    if (blocks > 0x7FFFFFFFull) {
        set_error("pipck_fwd_rewrite_ring: too many slots for one launch");
        return PIPCK_ERANGE;
    }
    PIPCK_LAUNCH(k_fwd_ring, dim3((uint32_t)blocks), dim3(256), 0, s, (uint8_t*)d_arena, (uint32_t)stride, d_lens, n,
                 (const u32x4*)d_rules, n_rules, d_rule_of, flags, d_done, d_err);
    PIPCK_LAUNCHED("k_fwd_ring");
    return PIPCK_OK;
}

}  // namespace pipck

extern "C" {

int pipck_fwd_rewrite_ring(void* d_arena, uint64_t slot_stride, const uint16_t* d_lens, uint64_t n_slots,
                           const pipck_fwd_rule* d_rules, uint32_t n_rules, const uint32_t* d_rule_of, uint32_t flags,
                           uint8_t* d_done, uint32_t* d_err, void* stream) {
    return pipck::launch_ring_fwd(d_arena, slot_stride, d_lens, n_slots, d_rules, n_rules, d_rule_of, flags, d_done,
                                  d_err, pipck::as_stream(stream));
}

}  // extern "C"

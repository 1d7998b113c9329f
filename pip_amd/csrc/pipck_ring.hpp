// pipck_ring.hpp -- the slot-group streams over frames in fixed-size ring slots,
// shared by k_ring (pipck_rxdev.hip: pipck_rx_verify_ring_n) and k_ring_tx
// (pipck_txring.hip: pipck_tx_fill_ring).  A block of four waves owns kRingB
// consecutive slots and leaves, in its LDS, each slot's frame sum and header
// window; what the block then does with them (a verdict, a fill) is the
// kernel's.  The schedules are described at k_ring.  Everything here is
// __forceinline__: each kernel carries its own copy, and a second caller
// changes nothing in the first one's code.
#pragma once
#include "pipck_device.hpp"

namespace pipck {

constexpr uint32_t kRingB = 64;        // slots per block
constexpr uint32_t kRingCoopRows = 2;  // mean rows per slot from which the waves interleave

struct RingLds {
    u32x4 hdr[6][kRingB];  // chunk k of slot g's header window
    uint32_t sum[kRingB];  // slot g's LE residue sum
};

// Sum of v over each aligned group of S lanes (S = 8, 16, 32), valid in lane
// S / 2 of the group: two quad swaps, a half-row mirror (8), a row mirror
// (16), then row_bcast:15 into rows 1 and 3 (32) -- DPP only, no LDS trips.
template <int S>
__device__ __forceinline__ uint32_t group_total(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);  // row_half_mirror
    if (S >= 16) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false);  // row_mirror
    if (S >= 32) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15
    return v;
}

// Short frames: group gi = lane / S of load j takes slot j * (64 / S) + gi,
// lane k = lane % S its chunk k; this wave takes loads first, first + step, ...
// Lc: lane g holds slot g's readable bytes, fetched per load for the group's
// slot (a ds_bpermute, again at the reduce rather than held: registers set the
// wave count, and a ring of U loads is reloaded as it is consumed).
template <int S, int U>
__device__ __forceinline__ void ring_short(RingLds& t, buf_t rb, uint32_t stride, uint32_t nb, uint32_t Lc,
                                           uint32_t first, uint32_t step, int lane) {
    constexpr uint32_t P = 64u / S;  // slots per load
    const uint32_t k = (uint32_t)lane % S, gi = (uint32_t)lane / S;
    const uint32_t loads = (nb + P - 1) / P;  // <= S
    auto issue = [&](uint32_t j) -> u32x4 {
        uint32_t off = 0xFFFFFFF0u;  // past the block's loads, or the frame: no request
        if (j < loads) {             // wave-uniform
            const uint32_t g = j * P + gi;
            const uint32_t Lg = (uint32_t)__shfl((int)Lc, (int)g, 64);
            if (16u * k < Lg) off = g * stride + 16u * k;
        }
        return buf_load<true>(rb, off);
    };
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = issue(first + step * u);
    for (uint32_t j0 = first; j0 < loads; j0 += step * U) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t j = j0 + step * u;
            if (j < loads) {  // wave-uniform
                const uint32_t g = j * P + gi;
                const int hi = (int)__shfl((int)Lc, (int)g, 64) - 16 * (int)k;
                const u32x4 x = hi < 16 ? mask_tail(v[u], hi) : v[u];
                const uint32_t tot = group_total<S>(dot4(x, 0u));
                if (k == S / 2) t.sum[g] = tot;
                if (k < 6) t.hdr[k][g] = x;
            }
            v[u] = issue(j + step * U);
        }
    }
}

// Longer frames: item i of the block's stream = row r of slot g, for the
// slots' row counts R (lane g: R_g = ceil(chunks_g / 64); incl their inclusive
// prefix).  Slot of item i: the number of slots whose rows all come before it
// (a ballot popcount); its row: i minus the rows before the slot.  This wave
// takes items first, first + step, ... below end; its run partial is flushed
// (one wave reduce, an LDS add: slots may be shared between waves) when the
// slot changes.
template <int U>
__device__ __forceinline__ void ring_rows(RingLds& t, buf_t rb, uint32_t stride, uint32_t Lc, uint32_t incl,
                                          uint32_t excl, uint32_t first, uint32_t end, uint32_t step, int lane) {
    u32x4 v[U];
    // per ring entry, one scalar: slot g (6 bits) | row r << 6 (6 bits: <= 64 rows
    // in a 64 KiB slot) | slot bytes L << 12 (17 bits) -- three scalars per entry
    // would take the kernel past 80 SGPRs, which costs a block per CU
    uint32_t se[U];
    auto issue = [&](uint32_t i, int u) {
        uint32_t g = 0, r = 0, L = 0;
        if (i < end) {  // wave-uniform
            g = (uint32_t)__popcll(__ballot(incl <= i));
            r = i - (uint32_t)__builtin_amdgcn_readlane((int)excl, (int)g);
            L = (uint32_t)__builtin_amdgcn_readlane((int)Lc, (int)g);
        }
        se[u] = g | r << 6 | L << 12;
        const uint32_t c = 64u * r + (uint32_t)lane;
        v[u] = buf_load<true>(rb, 16u * c < L ? g * stride + 16u * c : 0xFFFFFFF0u);
    };
    auto flush = [&](uint32_t g, uint32_t acc) {
        const uint32_t s = wave_total(acc);
        if (lane == 0) atomicAdd(&t.sum[g], s);
    };
#pragma unroll
    for (int u = 0; u < U; u++) issue(first + step * u, u);
    uint32_t cur = 0xFFFFFFFFu, acc = 0;
    for (uint32_t j0 = first; j0 < end; j0 += step * U) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t i = j0 + step * u;
            if (i < end) {  // wave-uniform
                const uint32_t g = se[u] & 63u, r = (se[u] >> 6) & 63u, L = se[u] >> 12;
                if (g != cur) {  // this wave's share of the previous slot is all in
                    if (cur != 0xFFFFFFFFu) flush(cur, acc);
                    cur = g;
                    acc = 0;
                }
                u32x4 x = v[u];
                if (L < 1024u * (r + 1u)) {  // wave-uniform: the frame ends in this row (else no mask)
                    const int hi = (int)L - 16 * (int)(64u * r + (uint32_t)lane);
                    if (hi < 16) x = mask_tail(x, hi);
                }
                acc = dot4(x, acc);
                if (r == 0 && lane < 6) t.hdr[lane][g] = x;
            }
            issue(i + step * U, u);  // past this wave's items: no request
        }
    }
    if (cur != 0xFFFFFFFFu) flush(cur, acc);
}

}  // namespace pipck

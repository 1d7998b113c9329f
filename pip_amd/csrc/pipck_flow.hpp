// pipck_flow.hpp -- a packet's flow, pseudo-header base, result and refusal: the
// one definition of each, for every batch kernel.  Plain integer code: under a
// plain C++17 compiler it includes nothing of HIP and every function is `inline`
// (tests/test_flow_rules.py pins it on a CPU through tests/flow_rules_main.cpp).
#pragma once
#include <stdint.h>

#include <type_traits>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define PIPCK_FN __host__ __device__ __forceinline__
#else
#define PIPCK_FN inline
#endif

namespace pipck {

PIPCK_FN uint32_t fold32(uint32_t x) { return (x & 0xFFFFu) + (x >> 16); }
// pip_fold_uint32 applied twice (pip_checksum.cpp:29-30); result in [0, 0xFFFF]
PIPCK_FN uint32_t fold16(uint32_t x) { return fold32(fold32(x)); }

// ~(u16)fold(fold(P + F)) -- the two folds of pip_standard_checksum
// (pip_checksum.cpp:29-30) and the final ~ of pip_inet_checksum (:60),
// pip_inet6_checksum (:86), pip_inet_checksum_buf (:114), pip_inet6_checksum_buf (:147)
PIPCK_FN uint16_t finish(uint32_t pseudo_total, uint32_t be_sum) { return (uint16_t)~fold16(pseudo_total + be_sum); }

// The implicit flow of packet i (no flow_of), the definition: "flow_origin + i is
// taken modulo 2^64 (a u64 sum that wraps) before the reduction modulo n_flows"
// (include/pipck.h).  The forms below compute exactly this; n_flows >= 1 in all.
PIPCK_FN uint32_t implicit_flow(uint64_t flow_origin, uint64_t i, uint32_t n_flows) {
    return (uint32_t)((flow_origin + i) % n_flows);
}

// A stepping walk: the flows of indices first, first + step, first + 2 step, ...
// from one 64-bit modulo, the step reduced once, a conditional subtract per step.
// PRECONDITION: no index of the walk passes 2^64 -- a remainder stepped across
// the wrap is wrong unless n_flows divides 2^64.  launch_fixed guarantees it: it
// launches a batch that crosses the wrap as two.  `implicit` false: stays at 0.
// k_fixed walks with it.  k_small, k_flat_small and k_flat_tiny spell the same walk
// out (steps 64, 256 and 1): each orders the two reductions its own way, the
// compiler keeps that order, and their code is held fixed.
struct FlowWalk {
    uint32_t flow = 0, step = 0, n_flows;
    PIPCK_FN FlowWalk(bool implicit, uint64_t flow_origin, uint64_t first, uint64_t step_, uint32_t n_flows_)
        : n_flows(n_flows_) {
        if (implicit) {
            flow = implicit_flow(flow_origin, first, n_flows);
            step = (uint32_t)(step_ % n_flows);
        }
    }
    PIPCK_FN void next() {
        flow += step;
        if (flow >= n_flows) flow -= n_flows;
    }
};

// The tile form (k_packed, k_packedb): the flow of index 64 tile + lane, lane in
// [0, 64), from one 64-bit modulo per tile.  x0 = flow_origin + 64 tile (modulo
// 2^64); the lanes from 2^64 - x0 on have an index that wrapped: it is
// lane - (2^64 - x0), not x0 + lane.  In two steps: the tile's modulo up front
// (wave-uniform), the lane's 32-bit one only where no flow_of entry replaces it.
struct TileFlow {
    uint32_t fl, n_flows;  // fl: the lane's flow before its last reduction, < n_flows + 64
    PIPCK_FN TileFlow(uint64_t flow_origin, uint64_t tile, uint32_t lane, uint32_t n_flows_) : n_flows(n_flows_) {
        const uint64_t x0 = flow_origin + tile * 64;
        const uint32_t f0 = (uint32_t)(x0 % n_flows);
        const uint64_t to_wrap = 0 - x0;
        fl = (uint64_t)lane >= to_wrap ? lane - (uint32_t)to_wrap : f0 + lane;
    }
    PIPCK_FN uint32_t flow() const { return fl % n_flows; }
};

// The task form (flat_pseudo): the flow of index p0 + lane, lane in [0, 64).
// A 32-bit remainder where the task's indices f0 .. f0 + 63 all fit (wave-uniform
// test): the 64-bit one is ~100 instructions.  The test is on f0 itself: f0 + 64
// can wrap past 2^64 and look small while f0 + lane has not.
PIPCK_FN uint32_t task_flow(uint64_t flow_origin, uint64_t p0, uint32_t lane, uint32_t n_flows) {
    const uint64_t f0 = flow_origin + p0, f = f0 + (uint64_t)lane;  // modulo 2^64, as pipck.h states
    return f0 <= 0xFFFFFFFFull - 64u ? (uint32_t)f % n_flows : (uint32_t)(f % n_flows);
}

// Pseudo-header base of a packet whose flow is f (a flow_of entry, a descriptor's
// flow or an implicit flow).  nf = the table's entries in the bounded _n forms
// (UINT32_MAX in the plain ones: trusted).  pip has no flow index to go stale --
// it passes the addresses by value on every call (pip_checksum.cpp:42,63) -- so
// an entry past the table is this engine's own failure mode and must never
// become a read outside the table: `bad` is set, the table is not read, and the
// caller stores 0 for that packet (packet_result) and reports it with refuse().
PIPCK_FN uint32_t flow_pseudo(const uint32_t* pseudo, uint32_t f, uint32_t nf, bool& bad) {
    bad = f >= nf;
    return bad ? 0u : pseudo[f];
}

// Report a refused packet, descriptor or tile: 1 << PIPCK_ERANGE in *err, where
// the caller gave one.  `refused`: for callers that hold the condition as a value.
constexpr uint32_t kErrRange = 1u << 2;  // 1 << PIPCK_ERANGE (include/pipck.h; asserted in pipck_kernels.hip)
PIPCK_FN void refuse(uint32_t* err, bool refused = true) {
#ifdef __HIP_DEVICE_COMPILE__
    if (refused && err) atomicOr(err, kErrRange);
#else
    if (refused && err) *err |= kErrRange;
#endif
}

// A packet's result from its pseudo-header total P and its big-endian folded sum
// F: 0 when refused; else the RX verdict (valid iff the sum including the checksum
// field folds to 0xFFFF) or the checksum.  T: the type the caller stores or packs,
// by default what the result is: bool, uint16_t.
template <bool VERIFY, class T = std::conditional_t<VERIFY, bool, uint16_t>>
PIPCK_FN T packet_result(uint32_t P, uint32_t F, bool bad) {
    if constexpr (VERIFY)
        return bad ? (T)0 : (T)(fold16(P + F) == 0xFFFFu);
    else
        return bad ? (T)0 : (T)finish(P, F);
}
// The same as a u32, computed first and then forced to 0, with the refusal reported
// on the spot: for the kernels that store the result afterwards (k_packed, k_packedb).
template <bool VERIFY>
PIPCK_FN uint32_t packet_result(uint32_t P, uint32_t F, bool bad, uint32_t* err) {
    uint32_t r = packet_result<VERIFY>(P, F, false);
    if (bad) {
        r = 0;
        refuse(err);
    }
    return r;
}

}  // namespace pipck

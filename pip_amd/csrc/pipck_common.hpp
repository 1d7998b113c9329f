// pipck_common.hpp -- host-side plumbing shared by the libpipck.so sources.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <memory>
#include <string>

#include "../../include/pipck.h"
#include "pipck_testing.h"
#include "pipck_tune.hpp"

namespace pipck {

void set_error(const std::string& msg);

// Map a HIP failure to PIPCK_EHIP with a message naming the call site.
inline int hip_fail(hipError_t e, const char* what) {
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return PIPCK_EHIP;
}

#define PIPCK_HIP(call)                                   \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return ::pipck::hip_fail(e_, #call); \
    } while (0)

// After a kernel launch: report launch-configuration errors synchronously.
#define PIPCK_LAUNCHED(name)                              \
    do {                                                  \
        hipError_t e_ = hipGetLastError();                \
        if (e_ != hipSuccess) return ::pipck::hip_fail(e_, name); \
    } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// The batch kernel this thread launched last (its host-side handle), so a
// measurement can name the exact template instantiation it timed
// (pipck_last_launch in pipck_testing.h: bench.py binds a PMC traffic file to
// that name).  One thread-local store per launch.
extern thread_local const void* t_last_kernel;
#define PIPCK_LAUNCH(K, ...)                                          \
    do {                                                              \
        ::pipck::t_last_kernel = reinterpret_cast<const void*>(K);    \
        hipLaunchKernelGGL(K, __VA_ARGS__);                           \
    } while (0)

// The batch kernels' n_flows argument: the modulus without flow_of (never 0);
// with it, the bound of its entries -- the caller's n_flows in the bounded _n
// forms, UINT32_MAX (trusted) in the plain forms and for an _n call that gives
// n_flows 0 (include/pipck.h: "n_flows 0: the entries are trusted").
inline uint32_t kernel_n_flows(const uint32_t* d_flow_of, uint32_t n_flows, bool bounded) {
    return d_flow_of ? (bounded && n_flows ? n_flows : UINT32_MAX) : (n_flows ? n_flows : 1u);
}

// Number of CUs on the current device (cached per device).
int device_cus();

// Registry of the pinned host ranges the GPU may read in place (made by
// pipck_host_alloc / pipck_host_register).  Zero-copy TX segments are checked
// against it at add time: a kernel touching an unpinned host page would fault
// the GPU, so a bad pointer must fail as PIPCK_EINVAL instead.  A queue that
// records a segment for an in-place read also HOLDS the segment's range until
// that batch completes: pipck_host_free / pipck_host_unregister refuse a held
// range (PIPCK_EBUSY), so no range can be released while the GPU may read it.
struct PinnedRec {
    uintptr_t lo = 0, hi = 0;  // [lo, hi)
    // holders in the low bits, kPinnedRemoved once released: one atomic word,
    // so "acquire unless removed" and "remove unless held" cannot interleave
    std::atomic<uint64_t> state{0};
};
constexpr uint64_t kPinnedRemoved = 1ull << 63;
using PinnedRef = std::shared_ptr<PinnedRec>;
void pinned_add(const void* p, size_t bytes);
// PIPCK_OK, PIPCK_EINVAL (not a range start) or PIPCK_EBUSY (held by a queued batch)
int pinned_remove(const void* p);
// The range holding all of [p, p+len), or null.
PinnedRef pinned_lookup(const void* p, size_t len);
// Take / drop one hold; acquire fails once the range has been removed.
bool pinned_acquire(PinnedRec& r);
void pinned_release(PinnedRec& r);

// pipck_checksum_chains without argument checks, for callers whose segment
// descriptors hold absolute device-accessible addresses (d_arena == nullptr):
// the TX queue mixes its device staging copy with zero-copy pinned host segments.
int chains_unchecked(const void* d_arena, const pipck_desc* d_segs, uint64_t n_segs, const uint64_t* d_seg_begin,
                     const uint32_t* d_pkt_flow, uint64_t n_packets, const uint32_t* d_pseudo, uint32_t* d_scratch,
                     uint16_t* d_out, uint32_t* d_err, hipStream_t s, uint64_t arena_bytes = UINT64_MAX,
                     uint32_t n_flows = UINT32_MAX);

// The launch functions below take the caller's snapshot of the tuning state
// (pipck_tune.hpp): rows, ring, load policy and the kernels' flag word come from it.

// The block-cooperative flat stream (pipck_coop.hip); PIPCK_EINVAL when the
// shape does not fit its block tasks (the caller then takes k_flat).
int launch_flat_coop(bool verify, const void* d_arena, uint64_t stride, uint32_t len, uint64_t n,
                     const uint32_t* d_pseudo, uint32_t n_flows, const uint32_t* d_flow_of, uint64_t flow_origin,
                     uint16_t* d_out, uint8_t* d_ok, uint32_t* d_err, hipStream_t s, const TuneView& tv);

// The header row stream (pipck_hdr.hip): 20/24-byte strides, no pseudo-header;
// PIPCK_EINVAL when the shape or the batch size does not fit (the caller then
// takes k_small).
int launch_hdr(bool verify, const void* d_arena, uint64_t stride, uint32_t len, uint64_t n, uint16_t* d_out,
               uint8_t* d_ok, hipStream_t s, const TuneView& tv);

// pipck_rx_verify_device (pipck_packedb.hip): k_packedb with the RX verdicts.
int launch_ring_rx(const void* d_arena, uint64_t stride, const uint16_t* d_lens, uint64_t n, uint8_t* d_ok,
                   uint32_t* d_err, hipStream_t s);
int launch_packedb_rx(const void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens, const uint64_t* d_tile_off,
                      uint64_t n, uint8_t* d_ok, uint32_t* d_err, hipStream_t s);
// pipck_tx_fill_ring (pipck_txring.hip): k_ring's streams with the TX fill at each block's end.
int launch_ring_tx(void* d_arena, uint64_t stride, const uint16_t* d_lens, uint64_t n, uint32_t flags,
                   uint8_t* d_done, uint32_t* d_err, hipStream_t s);
// pipck_fwd_rewrite_ring (pipck_fwd.hip): NAT and TTL rewrite of ring slots from their headers alone.
int launch_ring_fwd(void* d_arena, uint64_t stride, const uint16_t* d_lens, uint64_t n, const pipck_fwd_rule* d_rules,
                    uint32_t n_rules, const uint32_t* d_rule_of, uint32_t flags, uint8_t* d_done, uint32_t* d_err,
                    hipStream_t s);

// The one-packet-per-wave measurement arm (pipck_wave.hip; TuneView::wave_arm()):
// fixed strides (desc == false) or descriptors.
int launch_wave(bool verify, bool desc, const void* d_arena, uint64_t stride, uint32_t len, const pipck_desc* d_desc,
                uint64_t n, const uint32_t* d_pseudo, uint32_t n_flows, const uint32_t* d_flow_of,
                uint64_t flow_origin, uint16_t* d_out, uint8_t* d_ok, uint32_t* d_err, hipStream_t s,
                uint32_t max_chunks, const TuneView& tv, uint64_t arena_bytes = UINT64_MAX);

}  // namespace pipck

// pipck_tune.hpp -- the one place that knows the layout of the internal tuning
// words (pipck_tune, pipck_tune_ring, pipck_tune_probes; pipck_testing.h) and
// the one decoder of them (TuneView).  Host and device code both include it:
// the constants are plain constexpr, and a kernel's `kflags` argument is the
// raw pipck_tune flags word (k_hdr, k_ring: their own words, below).
//
// Two other files spell the same layout and tests/test_tune_layout.py holds
// them to this one: the tables in pipck_testing.h and TUNE_BITS in
// pip_amd/engine.py.  The test reads the `constexpr uint32_t k... = ...;`
// lines between the `// @word` markers, so keep one constant per line.
#pragma once
#include <stdint.h>

#include <initializer_list>

namespace pipck {

// @word lanes -- pipck_tune's lanes_per_packet: 1..64 = k_fixed's group width, or
// the one-packet-per-wave measurement arm (pipck_wave.hip): fixed strides and
// descriptor batches take k_wave, the ring verifier k_ring_slots.
constexpr uint32_t kWaveArm = 256;

// @word flags -- pipck_tune's flags.  Every setting computes the same results
// except the measurement bits 21-23.
// Load policy: bit 0 forces plain (cached) loads, bit 2 non-temporal ones;
// otherwise each kernel uses what measured faster on MI355X
// (profiles/README.md): nt for the streaming kernels, plain for small groups.
constexpr uint32_t kPlainLoads = 1u << 0;
constexpr uint32_t kNtLoads = 1u << 2;
constexpr uint32_t kNoFlat = 1u << 1;  // never the flat-stream fixed kernels (k_flat, k_flat_coop)
// XCD-grouped task split (xcd_tasks in pipck_kernels.hip; off by default, speed only)
constexpr uint32_t kXcdGroups = 1u << 3;
constexpr uint32_t kNoPackedTiles = 1u << 4;  // ragged tiles always take the lookup path
constexpr uint32_t kWideBlocks = 1u << 5;     // 4-wave ragged blocks instead of 1-wave
constexpr uint32_t kNoSmall = 1u << 6;        // never the small-packet kernel
constexpr uint32_t kNoFlatSmall = 1u << 7;    // never the short-stride flat kernel
// bits 8..15: 1 KiB rows per wave task of the row-stream kernels (0 = each kernel's default)
constexpr uint32_t kRowsShift = 8;
constexpr uint32_t kRowsField = 0xFFu << 8;
constexpr uint32_t kNoTinyTiles = 1u << 16;    // tiny ragged tiles take the chunk stream too
constexpr uint32_t kNoFlatTiny = 1u << 17;     // never k_flat_tiny
constexpr uint32_t kForceFlatTiny = 1u << 18;  // k_flat_tiny without pseudo-headers too
// mixed rows of packed ragged tiles always take the LDS marks (k_ragged; in
// k_packed the marks are the default and this bit selects the scalar end loop)
constexpr uint32_t kPackedMarksOnly = 1u << 19;
// The streaming kernels record, per wave task, the 100 MHz wall clock
// (s_memrealtime) when the task starts and when its results are stored, plus
// the wave's hardware slot, so tools/task_trace.py can see the launch ramp, the
// tail, per-XCD progress and the gap between consecutive tasks on one wave
// slot.  One 32-byte vector store per task; off by default.
constexpr uint32_t kTrace = 1u << 20;
// MEASUREMENT ONLY, wrong results: the flat kernels' rows are waited for and
// consumed by one add each, with no per-packet work, so tools can time the
// access pattern alone.  (Bits 24..27 are the small kernel's packets per lane:
// this bit must not overlap them.)
constexpr uint32_t kLoadsOnly = 1u << 21;
// MEASUREMENT ONLY, no results: k_flat / k_flat_coop skip their task end (the
// per-packet LDS sums, pseudo-header add and result stores)
constexpr uint32_t kNoTaskEnd = 1u << 22;
// MEASUREMENT ONLY, no results: k_flat's task end computes every result but stores none
constexpr uint32_t kEndNoStore = 1u << 23;
// bits 24..27: k_small's packets per lane K (1 = 2, 2 = 4, 3 = 8, 4 = 16);
// default 2: deeper tasks measured slower (cfg1 at 64M-256M headers: K = 2 / 4
// / 8 / 16 -> 4.19 / 4.15 / 3.83 / 3.87 TB/s, plain loads beat nt by 10 %,
// profiles/r01_small_kernel_scan.jsonl)
constexpr uint32_t kSmallDepthShift = 24;
constexpr uint32_t kSmallDepthField = 0xFu << 24;
// The other fixed-stride schedule (same results): k_flat (one task per wave)
// instead of the block-cooperative k_flat_coop (pipck_coop.hip), the default
// for strides from 1 KiB to 64 KiB since round 4 -- except exactly 1 and 2 KiB,
// where it is the reverse; for the ring verifier, the row stream k_ring_rx
// instead of k_ring.
constexpr uint32_t kAltSchedule = 1u << 28;
// k_flat / k_packed store their results with plain write-back stores (the r02
// policy) instead of the write-through sc1 stores (store_result16)
constexpr uint32_t kPlainResultStores = 1u << 29;
// EXPERIMENTAL (same results): per-wave result stores in k_flat (the r02 scheme)
// instead of one coalesced store of the whole block's results by its last wave
constexpr uint32_t kFlatWaveStores = 1u << 30;
// k_packed: tile rows on the r02 grid (from the tile's first chunk) instead of the 128-B line grid
constexpr uint32_t kPackedNoAlign = 1u << 30;
// k_flat: wave tasks of exactly the packet count the heuristic names, not rounded to a multiple of 16
constexpr uint32_t kFlatFreeRun = 1u << 31;
// k_hdr reads bits 29-31 as its result-store policy (same results): plain
// write-back, non-temporal (default: write-through, sc1), one store per result
// instead of 16-byte pieces
constexpr uint32_t kHdrPlainStores = 1u << 29;
constexpr uint32_t kHdrNtStores = 1u << 30;
constexpr uint32_t kHdrNarrowStores = 1u << 31;
// @word private -- bits of a kernel's own flag word that pipck_tune never sets.
// k_hdr, measurement only (pipck_tune_probes, not a tune
// flag -- the flags' settings all compute the same results): store each
// header's checksum INTO the header -- htons(result) at byte 10, its ip_sum, as
// pip_netif.cpp:97 stores it -- instead of into the result array (which is left
// untouched): the "results inside the headers" layout, to weigh its write-back
// of whole dirty lines against the separate 2-byte result stream.  launch_hdr
// sets it from the probes word and clears whatever the tune flags hold there.
constexpr uint32_t kHdrInPlace = 1u << 28;

// @word probes -- pipck_tune_probes: measurement-only probes that change results
constexpr uint32_t kProbeHdrInPlace = 1u << 0;

// @word ring -- pipck_tune_ring: k_ring's schedule switches, a word of their own
// (they once shared pipck_tune's flag bits 27 / 29 with the small
// kernel's depth and the result-store policy)
constexpr uint32_t kRingOwnSlots = 1u << 0;  // the row stream never interleaves its waves
constexpr uint32_t kRingAllCoop = 1u << 1;   // the row stream always interleaves them
constexpr uint32_t kRingNoAdapt = 1u << 2;   // no feedback: k_ring at every fill (the round-5 default)
constexpr uint32_t kRingAdaptAll = 1u << 3;  // the feedback at every slot stride (tests; default from 4 KiB)

// @word masks -- the bits each kernel family reads.  Inside one family's word
// every bit has one meaning (the static_asserts); ACROSS families bits 28-31 are
// reused on purpose, and this is the only place that says so:
//   bit 28  the other schedule for launch_fixed and the ring verifier; in k_hdr's
//           own word the in-place probe (launch_hdr overwrites it)
//   bit 29  plain result stores for k_flat / k_packed and for k_hdr
//   bit 30  k_flat per-wave stores | k_packed r02 row grid | k_hdr nt stores
//   bit 31  k_flat free run | k_hdr one store per result
constexpr uint32_t kLoadPolicy = kPlainLoads | kNtLoads;  // every family
constexpr uint32_t kProbeBits = kLoadsOnly | kNoTaskEnd | kEndNoStore;
// which fixed-stride kernel (launch_fixed; host only)
constexpr uint32_t kFixedSelectWord = kLoadPolicy | kNoFlat | kNoSmall | kNoFlatSmall | kNoFlatTiny | kForceFlatTiny |
                                      kSmallDepthField | kAltSchedule;
constexpr uint32_t kFlatWord = kLoadPolicy | kXcdGroups | kRowsField | kTrace | kProbeBits | kPlainResultStores |
                               kFlatWaveStores | kFlatFreeRun;
constexpr uint32_t kFlatCoopWord = kRowsField | kLoadsOnly | kNoTaskEnd;
constexpr uint32_t kFlatShortWord = kLoadPolicy | kXcdGroups | kRowsField;  // k_flat_small, k_flat_tiny
constexpr uint32_t kHdrWord = kLoadPolicy | kRowsField | kHdrInPlace | kHdrPlainStores | kHdrNtStores |
                              kHdrNarrowStores;
constexpr uint32_t kRaggedWord = kLoadPolicy | kXcdGroups | kNoPackedTiles | kWideBlocks | kNoTinyTiles |
                                 kPackedMarksOnly;
constexpr uint32_t kPackedWord = kLoadPolicy | kNoPackedTiles | kNoTinyTiles | kPackedMarksOnly | kTrace |
                                 kPlainResultStores | kPackedNoAlign;
constexpr uint32_t kRingWord = kRingOwnSlots | kRingAllCoop | kRingNoAdapt | kRingAdaptAll;
// @word end

constexpr bool bits_disjoint(std::initializer_list<uint32_t> bits) {
    uint32_t seen = 0;
    for (uint32_t b : bits) {
        if (seen & b) return false;
        seen |= b;
    }
    return true;
}
static_assert(bits_disjoint({kPlainLoads, kNtLoads, kNoFlat, kNoSmall, kNoFlatSmall, kNoFlatTiny, kForceFlatTiny,
                             kSmallDepthField, kAltSchedule}),
              "launch_fixed's selection bits overlap");
static_assert(bits_disjoint({kFixedSelectWord, kXcdGroups, kRowsField, kTrace, kLoadsOnly, kNoTaskEnd, kEndNoStore,
                             kPlainResultStores, kFlatWaveStores, kFlatFreeRun}),
              "k_flat's bits overlap each other or launch_fixed's");
static_assert((kFlatCoopWord & ~kFlatWord) == 0, "k_flat_coop reads a subset of k_flat's word, same meanings");
static_assert((kFlatShortWord & ~kFlatWord) == 0, "k_flat_small / k_flat_tiny read a subset of k_flat's word");
// k_hdr's word holds bit 28 as the in-place probe and 29-31 as the store policy, not k_flat's meanings
static_assert(bits_disjoint({kPlainLoads, kNtLoads, kRowsField, kHdrInPlace, kHdrPlainStores, kHdrNtStores,
                             kHdrNarrowStores}),
              "k_hdr's bits overlap");
static_assert((kHdrWord & (kSmallDepthField | kProbeBits | kTrace | kXcdGroups)) == 0,
              "k_hdr must not read a bit that means something else to the fixed-stride kernels");
static_assert(bits_disjoint({kPlainLoads, kNtLoads, kXcdGroups, kNoPackedTiles, kWideBlocks, kNoTinyTiles,
                             kPackedMarksOnly}),
              "k_ragged's bits overlap");
static_assert(bits_disjoint({kPlainLoads, kNtLoads, kNoPackedTiles, kNoTinyTiles, kPackedMarksOnly, kTrace,
                             kPlainResultStores, kPackedNoAlign}),
              "k_packed's bits overlap");
static_assert(bits_disjoint({kRingOwnSlots, kRingAllCoop, kRingNoAdapt, kRingAdaptAll}), "ring mode bits overlap");
static_assert((kSmallDepthField & (kLoadsOnly | kAltSchedule | kPlainResultStores)) == 0,
              "the small kernel's depth must stay clear of its neighbours (ADVICE r05)");

// The ring coding of loads_per_lane shared by k_flat and k_ragged: 2/4/8/16 =
// that many rows in flight, reduced and reloaded a batch at a time; U + 1 = a
// ring of U rows (each reduced row's registers take the load U rows ahead at
// once) for U = 2/4/6/8/12/16/24/32.  Anything else, and a kernel that has no
// such instantiation, gets `other` -- each kernel's own fall-through.
struct RingShape {
    uint32_t u;
    bool pipe;
};
constexpr RingShape ring_shape(uint32_t loads, RingShape other) {
    switch (loads) {
        case 2: case 4: case 8: case 16: return {loads, false};
        case 3: case 5: case 7: case 9: case 13: case 17: case 25: case 33: return {loads - 1, true};
        default: return other;
    }
}

// One launch's view of the tuning state.  tune_now() loads each word once, at
// the top of a launch function, and the view is passed down, so one launch
// never sees two settings.  (pipck_tune still must not race with launches: the
// view only keeps a launch consistent with itself.)
struct TuneView {
    uint32_t lanes, loads, blocks, flags, ring_mode, probes;
    bool has(uint32_t bit) const { return (flags & bit) != 0; }
    uint32_t rows() const { return (flags & kRowsField) >> kRowsShift; }                // 0 = the kernel's default
    uint32_t small_depth() const { return (flags & kSmallDepthField) >> kSmallDepthShift; }
    bool wave_arm() const { return lanes == kWaveArm; }
    bool alt_schedule() const { return has(kAltSchedule); }
    bool flat_allowed() const { return !has(kNoFlat); }
    uint32_t grid_cap() const { return blocks; }  // 0 = no cap
    // non-temporal loads?  `streaming`: what the kernel takes when neither policy bit is set
    bool nt(bool streaming) const { return has(kPlainLoads) ? false : (has(kNtLoads) ? true : streaming); }
    RingShape ring(RingShape deflt, RingShape other) const { return loads ? ring_shape(loads, other) : deflt; }
};
TuneView tune_now();  // pipck_kernels.hip, next to the words and their setters

}  // namespace pipck

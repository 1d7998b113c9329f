/*
 * pipck_testing.h -- INTERNAL tuning hook of libpipck.so, for the GPU tests and
 * the measurement tools only (tests/, tools/).  Not part of the public ABI in
 * include/pipck.h: it is process-global mutable state that changes kernel
 * selection for every context and thread, so a product caller must never
 * use it.  Every setting computes the same results (the GPU tests sweep them
 * against the oracle); only speed changes -- except bits 21-23 below,
 * measurement-only probes.  pipck_tune(0, 0, 0, 0) restores
 * the automatic choice.
 */
#ifndef PIPCK_TESTING_H
#define PIPCK_TESTING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Launch-shape override for tuning; 0 = automatic everywhere (process-wide,
 * internal).  A hook, not an API: it takes no lock, and a call must not race
 * with a launch on any thread (each launch reads the words once, so it is
 * consistent with itself, but which setting it sees is then undefined).
 * pip_amd/csrc/pipck_tune.hpp names every bit and decodes it (TuneView);
 * tests/test_tune_layout.py holds these tables and engine.tune() to it.
 *
 * lanes_per_packet
 *   1/2/4/8/16/32/64   k_fixed's lanes per packet (with loads_per_lane its
 *                      loads per lane); any nonzero value keeps fixed strides
 *                      off every other fixed-stride kernel
 *   256  kWaveArm      k_wave (pipck_wave.hip: one packet per wavefront, the
 *                      north_star's sketch, a measurement arm) for fixed
 *                      strides and descriptor batches, loads_per_lane
 *                      2/4/8/16 its chunks per lane per pass;
 *                      pipck_rx_verify_ring takes k_ring_slots
 * blocks               caps the grid (k_ring: see its table below)
 *
 * flags
 *   bit    name                read by                      meaning
 *   0      kPlainLoads         every batch kernel           plain (cached) loads
 *   2      kNtLoads            every batch kernel           non-temporal loads (default: per kernel)
 *   1      kNoFlat             launch_fixed                 never the flat-stream fixed kernels
 *   3      kXcdGroups          k_flat* k_ragged             XCD-grouped task split
 *   4      kNoPackedTiles      k_ragged k_packed            no packed-tile addressing
 *   5      kWideBlocks         k_ragged                     4-wave ragged blocks (default 1)
 *   6      kNoSmall            launch_fixed                 never the small-packet kernel (packets
 *                                                           <= 64 B incl. chunk offset)
 *   7      kNoFlatSmall        launch_fixed                 never the short-stride flat kernel
 *                                                           (16-B-multiple strides < 1 KiB)
 *   8..15  kRowsField          the row-stream kernels       1 KiB rows per wave task (kRowsShift;
 *                                                           defaults in the tables below)
 *   16     kNoTinyTiles        k_ragged k_packed            no lane-per-segment path for tiles of
 *                                                           tiny segments
 *   17     kNoFlatTiny         launch_fixed                 never the tiny-stride flat kernel
 *                                                           (8-B-multiple strides <= 64 B with
 *                                                           pseudo-headers or RX verify)
 *   18     kForceFlatTiny      launch_fixed                 that kernel without pseudo-headers too
 *   19     kPackedMarksOnly    k_ragged k_packed            mixed rows of packed tiles always find
 *                                                           segments through LDS marks (default: a
 *                                                           scalar loop over up to 4 segment ends
 *                                                           per row); k_packed: the reverse
 *   20     kTrace              k_flat k_packed              record the per-task timeline
 *                                                           (pipck_trace_tasks below)
 *   21     kLoadsOnly          k_flat k_flat_coop           MEASUREMENT ONLY, WRONG RESULTS: waits
 *                                                           for and consumes every row with one add
 *                                                           and does no per-packet work (times the
 *                                                           access pattern alone)
 *   22     kNoTaskEnd          k_flat k_flat_coop           MEASUREMENT ONLY, NO RESULTS: skips the
 *                                                           task end
 *   23     kEndNoStore         k_flat                       MEASUREMENT ONLY, NO RESULTS: computes
 *                                                           its results but stores none
 *   24..27 kSmallDepthField    k_small                      packets per lane (kSmallDepthShift;
 *                                                           1 = 2, 2 = 4, 3 = 8, 4 = 16; default 2)
 *   28     kAltSchedule        launch_fixed launch_ring_rx  the other schedule: k_flat (one task
 *                                                           per wave) instead of the block-
 *                                                           cooperative k_flat_coop, the default for
 *                                                           16-B-multiple strides from 1 KiB to 64
 *                                                           KiB except exactly 1 and 2 KiB (there
 *                                                           the reverse); pipck_rx_verify_ring: the
 *                                                           row stream k_ring_rx instead of k_ring
 *   29     kPlainResultStores  k_flat k_packed              result stores with the r02 write-back
 *                                                           policy instead of write-through (sc1)
 *   30     kFlatWaveStores     k_flat                       the r02 scheme: per-wave result stores
 *                                                           (default: one coalesced store per block)
 *   30     kPackedNoAlign      k_packed                     the r02 scheme: tile rows from the
 *                                                           tile's first chunk (default: from its
 *                                                           128-B line)
 *   31     kFlatFreeRun        k_flat                       tasks of exactly the packet count the
 *                                                           rows knob gives (default: a multiple of
 *                                                           16 for strides < 4 KiB)
 *   29     kHdrPlainStores     k_hdr                        result stores plain write-back
 *   30     kHdrNtStores        k_hdr                        result stores non-temporal (default
 *                                                           write-through sc1)
 *   31     kHdrNarrowStores    k_hdr                        one store per result instead of 16-byte
 *                                                           pieces
 *   28     kHdrInPlace         k_hdr (its own word only)    never from pipck_tune: launch_hdr sets it
 *                                                           from pipck_tune_probes (kProbeHdrInPlace)
 * Bits 21-23 (kProbeBits) isolate the task-end cost
 * (profiles/r03_flat_end_probe.jsonl).  They launch separate probe kernels
 * (k_flat_probe, k_flat_coop_probe: checksum mode, non-temporal loads, rings
 * 24/32 for k_flat); the production kernels have them compiled out and ignore
 * them otherwise.  Bits 29-31 compute the same results; they exist for the
 * separate-process A/Bs recorded in profiles/.  Bits 28-31 mean different
 * things to different kernel families on purpose: pipck_tune.hpp states the
 * reuse once and asserts that no family's word holds two meanings of a bit.
 *
 * loads_per_lane, rows (bits 8..15) and blocks, per kernel (0 = the default)
 *   k_fixed       loads_per_lane = loads per lane (with lanes_per_packet); blocks caps the grid
 *   k_flat        loads 2/4/8/16 = rows in flight, 3/5/9/13/17/25/33 = ring-pipelined
 *                 2/4/8/12/16/24/32 (default 25, from 4 KiB 33; anything else 8);
 *                 rows per wave task default 46, from 4 KiB 96
 *   k_flat_coop   loads >= 32 / >= 24 / other = ring 32 / 24 / 16 (17/25/33 in k_flat's
 *                 coding; default 32); rows per wave default 48, jumbo 64
 *   k_flat_small  rows per wave task default 64
 *   k_flat_tiny   loads 8 / 16 = its ring (default 4; 4 too); rows per wave task default 12
 *   k_hdr         (20/24-byte strides, no pseudo-header) loads 8/16/24/32 = its ring at any
 *                 batch size (default 32, from 8M headers), 9/17/25/33 = the same rings in
 *                 the block-cooperative row order, 1 = never k_hdr (k_small instead);
 *                 rows per wave task default 32
 *   k_ragged      loads as k_flat plus 7 = ring of 6 (in {2,4,8} rows in flight as for
 *                 k_flat; default 25; anything else a ring of 4)
 *   k_packed      (pipck_checksum_packed) loads 17/25/33 = a ring of 16/24/32 (default 32)
 *   k_packedb     (pipck_checksum_packed_bytes; default 8 waves per tile with rings of 3)
 *                 loads 32 = one wave per tile with a ring of 32 (the round-4 shape),
 *                 48 = 4 waves x 8, 72 / 74 = 8 waves x 2 / 4
 *   k_packedb_rx  (pipck_rx_verify_device; k_packedb_tx, pipck_tx_fill_device, alike;
 *                 default 4 waves with rings of 8) loads 32 = one wave x 32, 48 = 4 waves
 *                 x 8, 28 = 2 waves x 16
 *   k_ring        (pipck_rx_verify_ring) loads 8 / 12 / 16 / 24 = its loads in flight, 17 /
 *                 25 = 16 / 24 in the interleaved row stream only (default 8, interleaved
 *                 12); blocks 8 / 16 / 32 makes its interleaved row stream cover so many
 *                 slots at a time; its other switches are pipck_tune_ring's, below
 *   k_fwd_device  (pipck_fwd_rewrite_device) one shape, four tiles of 64 frames per block of
 *                 four independent waves: it reads no tune word */
void pipck_tune(uint32_t lanes_per_packet, uint32_t loads_per_lane, uint32_t blocks, uint32_t flags);

/* MEASUREMENT-ONLY probes that CHANGE RESULTS, kept apart from pipck_tune's
 * flags (whose settings all compute the same results; process-wide, internal).
 * Bit 0 (kProbeHdrInPlace) = k_hdr stores each IPv4 header's checksum into the header's ip_sum
 * (htons, byte 10, as pip_netif.cpp:97 stores it) and leaves the result array
 * untouched (the "results inside the headers" layout).
 * 0 switches every probe off. */
void pipck_tune_probes(uint32_t probes);

/* The ring verifier's schedule switches (pipck_rx_verify_ring; process-wide,
 * internal, every setting gives the same verdicts; 0 = automatic: k_ring, and
 * for slot strides from 4 KiB k_ring or the row stream k_ring_rx as the
 * feedback of the same ring's earlier launches says it is full): bit 0
 * (kRingOwnSlots) = k_ring's row stream never deals items round-robin to the
 * block's waves, bit 1 (kRingAllCoop) = always; bit 2 (kRingNoAdapt) = no
 * feedback (k_ring at every fill, the round-5 default); bit 3 (kRingAdaptAll)
 * = the feedback at every stride. */
void pipck_tune_ring(uint32_t mode);

/* XCD-weighted static deal for k_flat (ring 24, checksum; measurement arm,
 * VERDICT r03 item 7): the grid is cut into periods of 8 x period blocks and
 * in each XCD x (blocks b with b % 8 == x) keeps its first m[x] blocks; the kept
 * blocks take the tasks in dispatch order.  m = NULL or period = 0 switches it
 * off.  Same results; only the share of tasks per XCD changes. */
int pipck_tune_xcd_weights(const uint32_t* m, uint32_t period);

/* Per-task timeline for tools/task_trace.py: with tune flags bit 20 set, the
 * flat-stream (k_flat) and packed ragged (k_packed) kernels store one record
 * {u64 task, u64 t_start, u64 t_end, u64 XCC_ID << 32 | HW_ID} per wave task
 * (100 MHz s_memrealtime clock) into d_buf[task] for task < cap.  d_buf is
 * device memory; null switches recording off. */
int pipck_trace_tasks(void* d_buf, uint64_t cap);

/* The demangled name of the batch kernel the calling thread launched last --
 * the exact template instantiation, spelled as rocprofv3 names it (e.g.
 * "void pipck::k_flat<32, true, false, true, 4>(unsigned char const*, ...)").
 * bench.py attaches a PMC traffic file to a bench line only when the file was
 * measured on this kernel of this build.  PIPCK_EINVAL before any launch. */
int pipck_last_launch(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* PIPCK_TESTING_H */

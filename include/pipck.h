/*
 * pipck.h -- C ABI of the MI355X Internet-checksum engine (libpipck.so).
 *
 * The engine computes plumk97/pip's one's-complement checksum
 * (pip/pip_checksum.cpp) on AMD MI355X (gfx950) with hand-written HIP kernels.
 * Everything here is plain C: pointers, sizes, int status codes; no torch or
 * C++ types.  Two layers:
 *
 *   1. Batch ABI (device-resident, the performance path).  Packets already in
 *      HBM, results (host-order u16, exactly what pip returns before the
 *      caller's htons) written to HBM.  Stream-ordered, asynchronous.
 *   2. Host ABI (context-owned buffers).  Host batches are pipelined
 *      H2D -> kernel -> D2H on two HIP streams; single packets / pip_buf chains
 *      go through an exact-semantics kernel.  libpip_checksum_amd.so (the C++
 *      drop-in for pip's six functions, include/pip_checksum_amd.h) is built on
 *      this layer.
 *
 * Reference interface each entry point replaces is cited per declaration.
 * Result semantics are bit-exact with pip_checksum.cpp, including 0x0000 being
 * returned as-is (never mapped to 0xFFFF) and per-segment odd-byte padding of
 * chains (pip_checksum.cpp:110-112, :145-147).
 *
 * Domain of the batch ABI: every segment is at most 65535 bytes (the IPv4/IPv6
 * payload-length field).  In that domain pip's u32 accumulator can never wrap,
 * which lets the kernels sum in any order.  The host ABI has no length limit
 * and reproduces pip's mod-2^32 wrap exactly (pip_checksum.cpp:16-23).
 */
#ifndef PIPCK_H
#define PIPCK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define PIPCK_OK         0
#define PIPCK_EINVAL     1   /* bad argument (null pointer, zero flows, ...) */
#define PIPCK_ERANGE     2   /* a segment longer than 65535 bytes in a batch */
#define PIPCK_EHIP       3   /* a HIP runtime call failed; see pipck_last_error() */
#define PIPCK_ENODEV     4   /* no gfx950 device / HIP unavailable */
#define PIPCK_ENOMEM     5
#define PIPCK_EBUSY      6   /* a pinned range is still read in place by a queued TX batch */

#define PIPCK_MAX_SEG_LEN 65535u

/* Human-readable text of the last error on the calling thread. */
const char* pipck_last_error(void);
/* ABI version, (major << 16) | minor (PIPCK_VERSION_MAJOR / _MINOR of this
 * header; a minor step only adds entry points).  1.1: the RX verdicts are the
 * 3-bit PIPCK_RX_* values (7 = verified; 3 = nothing failed, payload NOT
 * checked) -- 1.0's single "ok == 3" meant verified.  1.2: the bounded _n forms
 * of the ragged, chain and ring calls.  1.3: the bounded _n forms of the
 * fixed-stride calls (pipck_checksum_fixed_n, pipck_verify_fixed_n,
 * pipck_update_fixed_n).  1.4: pipck_tx_fill_device.  1.5: pipck_tx_fill_ring.
 * 1.6: pipck_fwd_rewrite_ring.  1.7: pipck_fwd_rewrite_device.
 * 1.8: pipck_fwd_classify_ring, pipck_fwd_classify_device and the host
 * functions of their binding table (pipck_fwd_key_hash, pipck_fwd_table_build,
 * pipck_fwd_frame_key). */
#define PIPCK_VERSION_MAJOR 1
#define PIPCK_VERSION_MINOR 8
uint32_t pipck_version(void);

/* ---- flows / pseudo-headers ------------------------------------------ */
/* One flow = one (src, dst, proto) pseudo-header; packet i of a batch uses
 * flow  flow_of ? flow_of[i] : (flow_origin + i) % n_flows, where
 * flow_origin + i is taken modulo 2^64 (a u64 sum that wraps) before the
 * remainder.
 * Addresses are in network order exactly as in struct in_addr / in6_addr.  */
typedef struct pipck_flow4 {
    uint32_t src;      /* in_addr.s_addr */
    uint32_t dst;
    uint8_t  proto;    /* IPPROTO_TCP / IPPROTO_UDP / ... */
    uint8_t  pad[3];
} pipck_flow4;

typedef struct pipck_flow6 {
    uint8_t src[16];   /* in6_addr */
    uint8_t dst[16];
    uint8_t proto;
    uint8_t pad[3];
} pipck_flow6;

/* Reduce a device flow table to one u32 pseudo-header base per flow:
 * src hi+lo + dst hi+lo + proto (pip_checksum.cpp:46-55 for v4, :70-82 for v6).
 * The per-packet length term is added by the checksum kernels. */
int pipck_flows4_prepare(const pipck_flow4* d_flows, uint32_t n_flows, uint32_t* d_pseudo, void* stream);
int pipck_flows6_prepare(const pipck_flow6* d_flows, uint32_t n_flows, uint32_t* d_pseudo, void* stream);

/* ---- batch ABI (device pointers, stream-ordered) ----------------------- */
/* Streams and graphs.  Every call of this section that takes device pointers
 * and a stream only enqueues work on that stream -- kernels, and for
 * pipck_rx_verify_ring_n at most one memset -- and returns without waiting for
 * it: no host synchronisation, no work on any other stream, d_err OR-ed by the
 * kernels (never stored).  All of them may be captured into a graph
 * (hipStreamBeginCapture on `stream`) and the graph replayed on other
 * contents at the same addresses: pipck_flows4/6_prepare, the fixed, ragged,
 * packed, byte-packed and chain checksum / verify calls with and without _n,
 * pipck_packed_index, pipck_packed_bytes_index, pipck_update_fixed{,_n},
 * pipck_rx_verify_device, pipck_rx_verify_ring{,_n} (a capturing stream takes
 * the slot groups and keeps no per-ring state), pipck_tx_fill_device,
 * pipck_tx_fill_ring, pipck_fwd_rewrite_ring, pipck_fwd_rewrite_device,
 * pipck_fwd_classify_ring and pipck_fwd_classify_device.
 * Calls from several host threads on streams of their own are independent.
 * NOT capturable: pipck_gen_ragged_layout and pipck_gen_zipf_lengths (they
 * allocate and synchronise), and the whole host ABI (pipck_ctx_*,
 * pipck_host_*, pipck_txq_*, pipck_rxq_*, pipck_rx_verify), which owns its
 * streams and waits for them. */
/* d_pseudo == NULL selects pip_ip_checksum semantics (no pseudo-header,
 * pip_checksum.cpp:35-39).  Otherwise the result is
 *   ~fold(pseudo[flow] + hi16(len) + lo16(len) + sum16be(bytes))
 * which equals pip_inet_checksum / pip_inet6_checksum (pip_checksum.cpp:42-87)
 * and pip_inet{,6}_checksum_buf on a single-segment chain (:90-148).        */

/* Fixed stride: packet i = d_arena + i*stride, len bytes.  Any alignment.
 * The kernels load whole aligned 16-byte chunks, so the bytes from the 16-byte
 * boundary at or below d_arena to the one at or above the last packet's end
 * must be readable device memory (every hipMalloc / torch allocation is: they
 * are 256-byte granular); bytes outside the packets never affect a result. */
int pipck_checksum_fixed(const void* d_arena, uint64_t stride, uint32_t len, uint64_t n_packets,
                         const uint32_t* d_pseudo, uint32_t n_flows, const uint32_t* d_flow_of,
                         uint64_t flow_origin, uint16_t* d_out, void* stream);
/* Bounded form (replaces the same per-packet calls, pip_checksum.cpp:42-87,
 * where pip passes the addresses by value -- :42, :63 -- so no index of its
 * can go stale): with d_pseudo, n_flows must be > 0 (PIPCK_EINVAL otherwise),
 * and every d_flow_of entry is checked against it on the device.  A packet
 * whose entry is >= n_flows -- a stale or foreign flow index -- never reads
 * the pseudo-header table: its result is 0 and d_err (optional, device u32)
 * is OR-ed with (1 << PIPCK_ERANGE); every other packet's result is unchanged.
 * The plain name above trusts the entries (n_flows is then unused when
 * d_flow_of is given). */
int pipck_checksum_fixed_n(const void* d_arena, uint64_t stride, uint32_t len, uint64_t n_packets,
                           const uint32_t* d_pseudo, uint32_t n_flows, const uint32_t* d_flow_of,
                           uint64_t flow_origin, uint16_t* d_out, uint32_t* d_err, void* stream);

/* Ragged: one descriptor per packet. */
typedef struct pipck_desc {
    uint64_t offset;   /* byte offset of the packet (or segment) in the arena; any alignment */
    uint32_t len;      /* bytes, <= 65535 */
    uint32_t flow;     /* flow index (ignored when d_pseudo == NULL and for chain segments) */
} pipck_desc;

/* d_err (optional, device u32): OR-ed with (1 << PIPCK_ERANGE) when a
 * descriptor is out of domain; that packet's result is then 0.  This form
 * trusts the descriptors' offsets and flows (only len > 65535 is refused). */
int pipck_checksum_ragged(const void* d_arena, const pipck_desc* d_desc, uint64_t n_packets,
                          const uint32_t* d_pseudo, uint16_t* d_out, uint32_t* d_err, void* stream);
/* Bounded form: arena_bytes = the arena's size (readable from the 16-byte
 * boundary at or below d_arena to the one at or above d_arena + arena_bytes);
 * with d_pseudo, n_flows = its entries (> 0).  A descriptor whose bytes
 * [offset, offset + len) pass arena_bytes (overflow-safe), whose len exceeds
 * 65535 or whose flow is >= n_flows -- a stale or foreign descriptor -- is not
 * read: its result is 0 and d_err gets (1 << PIPCK_ERANGE).  The plain name
 * above is this with arena_bytes and n_flows unbounded. */
int pipck_checksum_ragged_n(const void* d_arena, uint64_t arena_bytes, const pipck_desc* d_desc, uint64_t n_packets,
                            const uint32_t* d_pseudo, uint32_t n_flows, uint16_t* d_out, uint32_t* d_err,
                            void* stream);

/* Packed ragged batch: per-packet lengths, no per-packet descriptors.
 * Packets lie back to back, each starting 16-byte aligned where the previous
 * one's bytes end rounded up to 16: packet i is at d_arena + 16 * c_i, with c_i
 * the sum of ceil(len_j / 16) over j < i (the layout of a TX staging arena and
 * of the synthetic cfg4 batches).  d_lens[i] = packet i's length (u16, so in
 * the batch domain by construction).  d_tile_chunk[t] = c_{64 t} for
 * t = 0 .. ceil(n/64) -- one u64 per 64 packets (pipck_packed_index builds it;
 * a producer that packs the arena knows it anyway) -- so the kernel reads 2 +
 * 1/8 bytes of metadata per packet instead of a 16-byte pipck_desc.  Flow of
 * packet i: d_flow_of ? d_flow_of[i] : (flow_origin + i) % n_flows; d_pseudo ==
 * NULL = pip_ip_checksum semantics.  Results as pipck_checksum_ragged
 * (pip_inet{,6}_checksum, pip_checksum.cpp:42-87).  d_arena 16-byte aligned;
 * a tile's loads start at the 128-byte line holding its first byte, so for an
 * arena that is not 128-byte aligned the bytes of its first line before
 * d_arena are loaded (same line, same page) and discarded. */
int pipck_checksum_packed(const void* d_arena, const uint16_t* d_lens, const uint64_t* d_tile_chunk,
                          uint64_t n_packets, const uint32_t* d_pseudo, uint32_t n_flows, const uint32_t* d_flow_of,
                          uint64_t flow_origin, uint16_t* d_out, void* stream);
/* RX verification of a packed batch (d_ok[i] = 1 iff packet i sums to 0xFFFF). */
int pipck_verify_packed(const void* d_arena, const uint16_t* d_lens, const uint64_t* d_tile_chunk,
                        uint64_t n_packets, const uint32_t* d_pseudo, uint32_t n_flows, const uint32_t* d_flow_of,
                        uint64_t flow_origin, uint8_t* d_ok, void* stream);
/* Bounded forms: arena_bytes = the arena's size (readable up to the 16-byte
 * boundary at or above it).  A tile of 64 packets whose chunks, as d_tile_chunk
 * and d_lens place them, reach past the arena -- a stale or foreign index --
 * is not read at all: each of its packets gets 0 (d_ok 0) and d_err (optional,
 * device u32) is OR-ed with (1 << PIPCK_ERANGE).  With d_flow_of and n_flows >
 * 0, an entry >= n_flows gives its packet 0 and sets the same bit (n_flows 0:
 * the entries are trusted).  The plain names above trust the index and the
 * flow entries (arena_bytes unbounded). */
int pipck_checksum_packed_n(const void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens,
                            const uint64_t* d_tile_chunk, uint64_t n_packets, const uint32_t* d_pseudo,
                            uint32_t n_flows, const uint32_t* d_flow_of, uint64_t flow_origin, uint16_t* d_out,
                            uint32_t* d_err, void* stream);
int pipck_verify_packed_n(const void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens,
                          const uint64_t* d_tile_chunk, uint64_t n_packets, const uint32_t* d_pseudo,
                          uint32_t n_flows, const uint32_t* d_flow_of, uint64_t flow_origin, uint8_t* d_ok,
                          uint32_t* d_err, void* stream);
/* Build d_tile_chunk (ceil(n/64) + 1 u64 entries; the last = the arena's 16-byte
 * chunks) from the lengths, on the stream. */
int pipck_packed_index(const uint16_t* d_lens, uint64_t n_packets, uint64_t* d_tile_chunk, void* stream);

/* Byte-packed ragged batch: packets back to back with NO padding -- packet i
 * at d_arena + b_i, b_i = len_0 + ... + len_{i-1} (a capture buffer, a
 * socket ring read in order, cfg4's bench layout).  d_tile_off[t] = b_{64 t}
 * for t = 0 .. ceil(n/64) (the last entry = the batch's bytes;
 * pipck_packed_bytes_index builds it), so the kernel reads 2 + 1/8 bytes of
 * metadata per packet and nothing but packet bytes otherwise (the 16-byte
 * granular layout above reads its padding too: 0.76 % of cfg4's bytes).
 * d_arena must be 128-byte aligned and readable up to the 16-byte boundary
 * after the last packet (any hipMalloc'd buffer of the batch's size is).
 * Flows and results as pipck_checksum_packed (pip_inet{,6}_checksum,
 * pip_checksum.cpp:42-87); any lengths 0..65535. */
int pipck_checksum_packed_bytes(const void* d_arena, const uint16_t* d_lens, const uint64_t* d_tile_off,
                                uint64_t n_packets, const uint32_t* d_pseudo, uint32_t n_flows,
                                const uint32_t* d_flow_of, uint64_t flow_origin, uint16_t* d_out, void* stream);
int pipck_verify_packed_bytes(const void* d_arena, const uint16_t* d_lens, const uint64_t* d_tile_off,
                              uint64_t n_packets, const uint32_t* d_pseudo, uint32_t n_flows,
                              const uint32_t* d_flow_of, uint64_t flow_origin, uint8_t* d_ok, void* stream);
/* Bounded forms, as pipck_checksum_packed_n: a tile whose bytes reach past
 * arena_bytes (readable to the 16-byte boundary at or above it) is not read;
 * its packets get 0 and d_err gets (1 << PIPCK_ERANGE); d_flow_of entries are
 * bounded by n_flows as there. */
int pipck_checksum_packed_bytes_n(const void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens,
                                  const uint64_t* d_tile_off, uint64_t n_packets, const uint32_t* d_pseudo,
                                  uint32_t n_flows, const uint32_t* d_flow_of, uint64_t flow_origin, uint16_t* d_out,
                                  uint32_t* d_err, void* stream);
int pipck_verify_packed_bytes_n(const void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens,
                                const uint64_t* d_tile_off, uint64_t n_packets, const uint32_t* d_pseudo,
                                uint32_t n_flows, const uint32_t* d_flow_of, uint64_t flow_origin, uint8_t* d_ok,
                                uint32_t* d_err, void* stream);
int pipck_packed_bytes_index(const uint16_t* d_lens, uint64_t n_packets, uint64_t* d_tile_off, void* stream);

/* Chains (pip_buf lists, pip_checksum.cpp:90-148): packet p owns segments
 * [d_seg_begin[p], d_seg_begin[p+1]); its pseudo-header length term is the
 * u32 sum of its segment lengths (pip_buf::total_len).  Every segment is
 * summed from its own start, exactly like pip's per-segment loop.
 * d_scratch: device u32[n_segs]. */
int pipck_checksum_chains(const void* d_arena, const pipck_desc* d_segs, uint64_t n_segs,
                          const uint64_t* d_seg_begin, const uint32_t* d_pkt_flow, uint64_t n_packets,
                          const uint32_t* d_pseudo, uint32_t* d_scratch, uint16_t* d_out, uint32_t* d_err,
                          void* stream);
/* Bounded form, as pipck_checksum_ragged_n for every segment (arena_bytes) and
 * every d_pkt_flow entry (n_flows, > 0 with d_pseudo): a packet holding a
 * refused segment, or with a flow past the table, gets 0 and d_err gets
 * (1 << PIPCK_ERANGE).  In both forms a packet whose [d_seg_begin[p],
 * d_seg_begin[p+1]) is not inside [0, n_segs] gets 0 and sets the same bit --
 * no segment record outside the scratch is read. */
int pipck_checksum_chains_n(const void* d_arena, uint64_t arena_bytes, const pipck_desc* d_segs, uint64_t n_segs,
                            const uint64_t* d_seg_begin, const uint32_t* d_pkt_flow, uint64_t n_packets,
                            const uint32_t* d_pseudo, uint32_t n_flows, uint32_t* d_scratch, uint16_t* d_out,
                            uint32_t* d_err, void* stream);

/* RX verification (a capability pip lacks): same
 * inputs as pipck_checksum_fixed but the packets carry their checksum field;
 * d_ok[i] = 1 when the one's-complement sum including the pseudo-header is
 * 0xFFFF (a valid packet), else 0. */
int pipck_verify_fixed(const void* d_arena, uint64_t stride, uint32_t len, uint64_t n_packets,
                       const uint32_t* d_pseudo, uint32_t n_flows, const uint32_t* d_flow_of,
                       uint64_t flow_origin, uint8_t* d_ok, void* stream);
/* Bounded form, as pipck_checksum_fixed_n: a refused packet verifies as 0. */
int pipck_verify_fixed_n(const void* d_arena, uint64_t stride, uint32_t len, uint64_t n_packets,
                         const uint32_t* d_pseudo, uint32_t n_flows, const uint32_t* d_flow_of,
                         uint64_t flow_origin, uint8_t* d_ok, uint32_t* d_err, void* stream);
/* The same for ragged batches (descriptors as for pipck_checksum_ragged);
 * out-of-domain descriptors verify as 0 and set d_err. */
int pipck_verify_ragged(const void* d_arena, const pipck_desc* d_desc, uint64_t n_packets,
                        const uint32_t* d_pseudo, uint8_t* d_ok, uint32_t* d_err, void* stream);
/* Bounded form, as pipck_checksum_ragged_n. */
int pipck_verify_ragged_n(const void* d_arena, uint64_t arena_bytes, const pipck_desc* d_desc, uint64_t n_packets,
                          const uint32_t* d_pseudo, uint32_t n_flows, uint8_t* d_ok, uint32_t* d_err, void* stream);

/* Incremental update for header rewrites (RFC 1624, SURVEY.md section 8 f4;
 * replaces a full re-run of pip_standard_checksum, pip_checksum.cpp:13-33,
 * after a field change).  Packet i at a = d_arena + i*stride carries pip's
 * checksum of the covered bytes a[cover_off, cover_off+cover_len) (an IPv4
 * header, or an L4 segment with flow pseudo-headers) as the big-endian u16 at
 * a + ck_off (htons(result), as pip's callers store it).  Bytes
 * a[edit_off, edit_off+edit_len) are replaced by d_new + i*new_stride, and
 * when d_pseudo_old / d_pseudo_new are given (prepared bases of the old and
 * new flow tables, e.g. a NAT address rewrite) the pseudo-header changes too;
 * the field is patched as  ~(~HC + ~m + m')  -- RFC 1624 eqn. 3.  The result
 * equals pip's full recomputation bit for bit (the 0x0000/0xFFFF corner eqn.
 * 3 cannot decide alone is settled by scanning that packet).
 * PIPCK_EINVAL unless: checksum field and edit lie in the cover at even
 * offsets from cover_off and do not overlap; edit_len is even or the edit
 * ends the cover; cover_off + cover_len <= stride; cover_len <= 65535. */
int pipck_update_fixed(void* d_arena, uint64_t stride, uint64_t n_packets, uint32_t cover_off, uint32_t cover_len,
                       uint32_t ck_off, uint32_t edit_off, uint32_t edit_len, const void* d_new,
                       uint64_t new_stride, const uint32_t* d_pseudo_old, const uint32_t* d_pseudo_new,
                       uint32_t n_flows, const uint32_t* d_flow_of, uint64_t flow_origin, void* stream);
/* Bounded form: with the pseudo-header tables, n_flows must be > 0 and bounds
 * every d_flow_of entry on the device.  A packet whose entry is >= n_flows is
 * left exactly as it was -- its edit bytes are not replaced and its checksum
 * field is not touched -- and d_err (optional, device u32) is OR-ed with
 * (1 << PIPCK_ERANGE).  The plain name above trusts the entries. */
int pipck_update_fixed_n(void* d_arena, uint64_t stride, uint64_t n_packets, uint32_t cover_off, uint32_t cover_len,
                         uint32_t ck_off, uint32_t edit_off, uint32_t edit_len, const void* d_new,
                         uint64_t new_stride, const uint32_t* d_pseudo_old, const uint32_t* d_pseudo_new,
                         uint32_t n_flows, const uint32_t* d_flow_of, uint64_t flow_origin, uint32_t* d_err,
                         void* stream);


/* ---- synthetic workloads (bench / tests; same spec as oracle/pipck_oracle.c) */
#define PIPCK_HDR_NONE 0
#define PIPCK_HDR_TCP  1
#define PIPCK_HDR_UDP  2
#define PIPCK_HDR_IPV4 3
uint64_t pipck_cfg_seed(uint32_t cfg);
/* packets [first_pkt, first_pkt+n) at d_arena + i*stride (any stride >= len); bytes [len,stride) zeroed */
int pipck_gen_fixed(void* d_arena, uint64_t stride, uint32_t len, uint64_t n, uint64_t first_pkt,
                    uint64_t seed, uint32_t hdr_kind, void* stream);
/* Zipf lengths 64..9000 for packets [first_pkt, first_pkt+n) -> d_len */
int pipck_gen_zipf_lengths(uint32_t* d_len, uint64_t n, uint64_t first_pkt, uint64_t seed, void* stream);
/* descriptors: offsets = exclusive prefix of roundup16(len); flow = (first_pkt+i) % n_flows.
 * *arena_bytes receives the arena size needed (synchronises the stream). */
int pipck_gen_ragged_layout(const uint32_t* d_len, uint64_t n, uint64_t first_pkt, uint32_t n_flows,
                            pipck_desc* d_desc, uint64_t* arena_bytes, void* stream);
int pipck_gen_ragged_fill(void* d_arena, const pipck_desc* d_desc, uint64_t n, uint64_t first_pkt,
                          uint64_t seed, uint32_t hdr_kind, void* stream);
/* byte-packed layout (pipck_checksum_packed_bytes): packets [first_pkt, first_pkt+n) with lengths d_lens */
int pipck_gen_packed_bytes(void* d_arena, const uint16_t* d_lens, const uint64_t* d_tile_off, uint64_t n,
                           uint64_t first_pkt, uint64_t seed, uint32_t hdr_kind, void* stream);
int pipck_gen_flows4(pipck_flow4* d_flows, uint32_t n_flows, uint64_t seed, uint8_t proto, void* stream);
int pipck_gen_flows6(pipck_flow6* d_flows, uint32_t n_flows, uint64_t seed, uint8_t proto, void* stream);

/* ---- host ABI ---------------------------------------------------------- */
typedef struct pipck_ctx pipck_ctx;

/* device < 0 selects the current HIP device. */
int pipck_ctx_create(int device, pipck_ctx** out);
int pipck_ctx_destroy(pipck_ctx* ctx);

/* One segment of a host-memory packet/chain. */
typedef struct pipck_hseg {
    const void* ptr;
    uint32_t len;
} pipck_hseg;

/* pip's exact sequential semantics over host bytes, computed on the device:
 *   sum = init; for each seg: sum = fold(fold((sum + sum16be(seg)) mod 2^32))
 * (pip_standard_checksum, pip_checksum.cpp:13-33, chained as at :110-112).
 * *out receives the final folded u32 in [0, 0xFFFF].  nseg == 0 behaves as one
 * empty segment (a pip_buf chain is never empty).  A segment with len == 0 may
 * have a null ptr and counts as empty; init is any u32 (the accumulator wraps
 * mod 2^32 with the data exactly as pip's does).  The 68 KiB of
 * pipck_ctx_zero_copy's modes 2-4 counts staged bytes, not payload bytes:
 * need = roundup16(16 * nseg) + sum of roundup16(len), a 16-byte table entry
 * per segment and every segment padded to 16 bytes.  Synchronous. */
int pipck_host_sum(pipck_ctx* ctx, const pipck_hseg* segs, uint32_t nseg, uint32_t init, uint32_t* out);

/* Host-resident fixed-stride batch: H2D in chunks, kernel, D2H of results,
 * double-buffered over two streams.  h_arena may be pageable or pinned
 * (pinned: see pipck_host_alloc).  Flows are host tables (v4 or v6, by family). */
int pipck_host_checksum_fixed(pipck_ctx* ctx, const void* h_arena, uint64_t stride, uint32_t len,
                              uint64_t n_packets, int family, const void* h_flows, uint32_t n_flows,
                              uint64_t flow_origin, uint16_t* h_out);
/* Host-resident byte-packed ragged batch (a capture buffer or a socket ring read
 * in order: packet i's h_lens[i] bytes right after packet i-1's, no padding),
 * the layout of pipck_checksum_packed_bytes: chunks of whole packets (~64 MiB)
 * go H2D with their lengths, are indexed and checksummed on the device, and the
 * results come back, double-buffered over two streams.  Flows, family and
 * results as pipck_host_checksum_fixed (h_out[i] = pip_inet{,6}_checksum /
 * pip_ip_checksum of packet i, host order).  Synchronous. */
int pipck_host_checksum_packed_bytes(pipck_ctx* ctx, const void* h_arena, const uint16_t* h_lens, uint64_t n_packets,
                                     int family, const void* h_flows, uint32_t n_flows, uint64_t flow_origin,
                                     uint16_t* h_out);
/* This context's per-packet path (pipck_host_sum): 0 = staged (H2D copy,
 * kernel, D2H copy), 1 = zero-copy (the kernel reads the pinned, coherent
 * staging buffer and writes the result to pinned host memory), 2 = auto
 * (zero-copy up to 68 KiB of staged bytes -- any single IP datagram; the
 * mode of a new context), 3 = resident (up to 68 KiB: one 256-thread block of this context stays on
 * the GPU, polls a doorbell in pinned host memory and answers without a
 * launch; it exits after 10 ms without a call, or when the mode changes or
 * the context is destroyed, and relaunches on the next call; larger calls take
 * the staged copies), 4 = resident with the doorbell in fine-grained device
 * memory the host writes directly (large-BAR systems; falls back to mode 3's
 * pinned doorbell where that allocation fails).  Every path computes the same
 * result.  Nothing is read from the environment.
 * WORST CASE of modes 3/4: while the resident block runs it holds one CU slot,
 * and HIP makes every hipFree / hipHostFree / hipDeviceSynchronize in the
 * whole process wait for it to exit -- up to 10 ms after this context's last
 * call (the idle exit).  pipck_ctx_zero_copy(ctx, 2) ends it at once. */
int pipck_ctx_zero_copy(pipck_ctx* ctx, int mode);
void* pipck_host_alloc(size_t bytes);   /* pinned, coherent host memory (device-readable in place) */
/* Pin an existing host range (a utun / socket buffer ring) so the GPU can read
 * it in place at the same address; PIPCK_EINVAL if the runtime maps it to a
 * different device address. */
int pipck_host_register(void* p, size_t bytes);
/* Both refuse (PIPCK_EBUSY, nothing released) while a TX queue holds segments
 * of the range for an in-place read that has not completed; PIPCK_EINVAL for a
 * pointer that does not start such a range. */
int pipck_host_unregister(void* p);
int pipck_host_free(void* p);

/* ---- deferred TX queue -------------------------
 * pip checksums each segment synchronously while building it
 * (pip/protocol/pip_tcp_packet.cpp:124-134, pip/protocol/pip_udp.cpp:50-51,
 * 60-61, pip/pip_netif.cpp:97).  A TX queue defers that: packets are added with
 * their bytes (the payloads of a pip_buf chain, in order), their pseudo-header
 * and the address of their 16-bit checksum field; pipck_txq_flush copies the
 * batch to the device, checksums all of it in one pass and stores
 * htons(result) into every field -- exactly the bytes pip would have written.
 * Bytes are copied at add time, so buffers may be reused after add; the
 * checksum fields must stay valid until flush.  One queue per thread. */
typedef struct pipck_txq pipck_txq;
int pipck_txq_create(pipck_ctx* ctx, pipck_txq** out);
int pipck_txq_destroy(pipck_txq* q);
/* pip_inet_checksum_buf (pip_checksum.cpp:90-115): src/dst as in_addr.s_addr */
int pipck_txq_add4(pipck_txq* q, const pipck_hseg* segs, uint32_t nseg, uint8_t proto, uint32_t src, uint32_t dst,
                   void* csum_field);
/* pip_inet6_checksum_buf (pip_checksum.cpp:118-148): src/dst as in6_addr bytes */
int pipck_txq_add6(pipck_txq* q, const pipck_hseg* segs, uint32_t nseg, uint8_t proto, const uint8_t* src,
                   const uint8_t* dst, void* csum_field);
/* Zero-copy forms: the segments lie in pinned host memory (pipck_host_alloc or
 * pipck_host_register) and are read by the GPU in place when the batch runs --
 * nothing is copied at add time, so they must stay valid and unchanged until
 * the batch completes (flush, or the complete/submit after its submit).  A
 * segment outside every such range is refused (PIPCK_EINVAL): the GPU must
 * never touch an unpinned host page. */
int pipck_txq_add4_zc(pipck_txq* q, const pipck_hseg* segs, uint32_t nseg, uint8_t proto, uint32_t src,
                      uint32_t dst, void* csum_field);
int pipck_txq_add6_zc(pipck_txq* q, const pipck_hseg* segs, uint32_t nseg, uint8_t proto, const uint8_t* src,
                      const uint8_t* dst, void* csum_field);
/* Automatic zero-copy, an explicit per-queue opt-in (off at creation; no
 * environment variable turns it on): pipck_txq_add4/add6 then read every
 * segment that lies in a pinned range in place and copy the others, so pinned
 * segments follow the zero-copy contract above -- the GPU reads them at flush
 * time, so they must stay valid and UNCHANGED until their batch completes.
 * Lets callers that cannot choose the _zc forms -- pip's deferred drop-in,
 * through pip_checksum_amd_zero_copy() -- use pinned utun/socket buffers
 * without a copy.  Every in-place segment holds its pinned range until its
 * batch completes (see pipck_host_free). */
int pipck_txq_auto_zero_copy(pipck_txq* q, int on);
/* Largest flush (staged bytes + metadata) this queue runs in place: the
 * kernels read the coherent pinned staging directly and write the results into
 * it, with no copy command.  Larger flushes take one H2D and one D2H copy.
 * Default 32 MiB (the measured crossover); 0 = always copy.
 * Per queue; no environment variable changes it. */
int pipck_txq_inplace_max(pipck_txq* q, uint64_t bytes);
/* pip_ip_checksum (pip_checksum.cpp:35-39): an IPv4 header with ip_sum = 0 */
int pipck_txq_add_ip(pipck_txq* q, const void* hdr, uint32_t len, void* csum_field);
/* packets added since the last submit/flush */
uint64_t pipck_txq_pending(const pipck_txq* q);
/* Synchronous: returns once every queued field holds its checksum; the queue is then empty. */
int pipck_txq_flush(pipck_txq* q);
/* Asynchronous flush, double-buffered: submit starts the queued batch (H2D,
 * kernels, D2H on the queue's stream) and returns; new adds go to a second
 * batch meanwhile.  complete waits for the submitted batch and stores its
 * fields.  At most one batch is in flight: submit first completes the previous
 * one.  Fields of a submitted batch hold their checksums only after the next
 * complete, submit or flush returns. */
int pipck_txq_submit(pipck_txq* q);
int pipck_txq_complete(pipck_txq* q);
/* packets submitted and not yet completed */
uint64_t pipck_txq_inflight(const pipck_txq* q);

/* ---- RX verification of received packets --------
 * pip never checks a received checksum (pip/pip_netif.cpp:45-77 hands packets
 * to TCP / UDP / ICMP as they come).  pipck_rx_verify checks n IP packets as
 * read from the tun device (IPv4 or IPv6, pkts[i] of lens[i] bytes, link
 * padding after the IP length allowed) in one call and sets ok[i]:
 *   PIPCK_RX_IP_OK       the IPv4 header checksum verifies (always set for IPv6)
 *   PIPCK_RX_L4_OK       no payload checksum failed: it verified, or there was
 *                        none this can check (PIPCK_RX_L4_CHECKED clear)
 *   PIPCK_RX_L4_CHECKED  the payload's checksum was computed: TCP / UDP over
 *                        their pseudo-headers (pip_inet{,6}_checksum), ICMPv4
 *                        over the message (pip_ip_checksum, RFC 792), ICMPv6
 *                        over the IPv6 pseudo-header, next header 58
 * ok[i] == PIPCK_RX_VERIFIED (7): both checksums computed and verified; 3:
 * nothing failed but the payload was NOT checked (an IPv4 or IPv6 fragment, an
 * IPv6 routing header, UDP over IPv4 with a zero checksum, another protocol);
 * malformed lengths or a truncated TCP/UDP/ICMP header leave the L4 bits
 * clear; not IPv4/IPv6, 0.  IPv6 hop-by-hop / destination-options headers and
 * atomic fragments are walked to the upper layer.  In full (tests/rx_reference.py
 * restates these rules in plain integer arithmetic and every path is held to it):
 *   - A frame under 20 bytes gets 0.  A version that is neither 4 nor 6 gets 0.
 *   - IPv4 with IHL < 5, total length < header length, or total length > frame
 *     length gets 0: no bit is set, PIPCK_RX_IP_OK included.  The header
 *     checksum covers the whole header, options included (IHL 6..15).
 *   - Version 6 with fewer than 40 bytes, or with 40 + payload length > frame
 *     length, gets 0.
 *   - An IPv4 fragment has MF or an offset set (ip_off & 0x3FFF != 0).  Its
 *     verdict is IP_OK (if the header verifies) plus L4_OK.
 *   - IPv6 walks next headers 0, 60 and 44 only.  A fragment header with an
 *     offset or M set (field & 0xFFF9) is unchecked (3).  A routing header (43)
 *     is unchecked (3).  A ninth extension header is unchecked (3), whatever it
 *     holds.  An extension header that does not fit in the payload gives IP_OK
 *     only.
 *   - The L4 length is the IP payload length from the upper-layer offset.  The
 *     UDP length field is not consulted.
 *   - An L4 length under 20 (TCP) or under 8 (UDP, ICMP) leaves the L4 bits clear.
 *   - UDP over IPv4 with a zero checksum field is unchecked (3).  UDP over IPv6
 *     with a zero field is checked like any other value.
 *   - Protocol 1 over IPv6 and protocol 58 over IPv4 are "another protocol" (3).
 *   - A checksum verifies when the one's-complement sum of its range is 0xFFFF:
 *     an all-zero ICMPv4 message (sum 0) fails.
 * Packets that lie in pinned
 * memory (pipck_host_alloc / pipck_host_register) are read in place by the GPU
 * and their ranges held until the call returns; others are copied.  Returns
 * when every ok[i] is set; *n_verified (optional) = packets with ok == 7.
 * One queue per thread (not thread-safe). */
#define PIPCK_RX_IP_OK 1u
#define PIPCK_RX_L4_OK 2u
#define PIPCK_RX_L4_CHECKED 4u
#define PIPCK_RX_VERIFIED 7u
typedef struct pipck_rxq pipck_rxq;
int pipck_rxq_create(pipck_ctx* ctx, pipck_rxq** out);
int pipck_rxq_destroy(pipck_rxq* q);
int pipck_rx_verify(pipck_rxq* q, const void* const* pkts, const uint32_t* lens, uint64_t n, uint8_t* ok,
                    uint64_t* n_verified);

/* The same verdicts for received IP packets already in DEVICE memory, in the
 * byte-packed layout of pipck_checksum_packed_bytes (frame i of d_lens[i]
 * bytes at d_arena + b_i, d_tile_off from pipck_packed_bytes_index; link
 * padding after the IP length allowed): d_ok[i] gets the PIPCK_RX_* bits
 * pipck_rx_verify gives the same bytes.  One kernel on `stream`, no host
 * work: the byte-packed stream sums every frame once, then a lane per packet
 * parses its headers and derives the IP-header and payload verdicts from that
 * sum.  The arena must be 128-byte aligned and readable to the 16-byte
 * boundary after the last frame.  Bounded as pipck_checksum_packed_bytes_n: a tile
 * reaching past arena_bytes is not read, its packets get 0 and d_err
 * (optional) gets (1 << PIPCK_ERANGE).  Asynchronous. */
int pipck_rx_verify_device(const void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens,
                           const uint64_t* d_tile_off, uint64_t n_packets, uint8_t* d_ok, uint32_t* d_err,
                           void* stream);

/* The same verdicts for frames in the fixed-size slots of a receive ring in
 * DEVICE memory: frame i of d_lens[i] bytes at d_arena + i * slot_stride, the
 * rest of each slot unused and never read.  d_arena 16-byte aligned, readable
 * for n_slots * slot_stride bytes; slot_stride a multiple of 16 from 1,024 to
 * 65,536 (PIPCK_EINVAL otherwise).  The lengths are bounded on the device: a
 * slot with d_lens[i] > slot_stride (a corrupt or foreign length) is not read
 * at all -- no load and no header parse leaves its slot -- gets d_ok[i] = 0,
 * and d_err (optional, device u32) gets (1 << PIPCK_ERANGE).  One kernel on
 * `stream`, asynchronous; d_ok[i] as pipck_rx_verify_device.  For slot strides
 * from 4 KiB the kernel's schedule follows the fill this ring (d_arena,
 * slot_stride) reported in earlier calls -- a row stream for full slots,
 * slot groups otherwise; the verdicts are the same either way.  The first call
 * on a ring allocates 8 bytes of device and 16 of pinned host memory that stay
 * with the library (at most 64 rings remembered). */
int pipck_rx_verify_ring_n(const void* d_arena, uint64_t slot_stride, const uint16_t* d_lens, uint64_t n_slots,
                           uint8_t* d_ok, uint32_t* d_err, void* stream);
/* pipck_rx_verify_ring_n without the error word (slots are bounded the same way). */
int pipck_rx_verify_ring(const void* d_arena, uint64_t slot_stride, const uint16_t* d_lens, uint64_t n_slots,
                         uint8_t* d_ok, void* stream);

/* The same verdicts for received frames back to back in HOST memory (a receive
 * buffer read in order, a capture file's records): chunks of ~64 MiB go H2D by
 * DMA with their u16 lengths, pipck_rx_verify_device judges them, the verdicts
 * come back; double-buffered over the context's two streams, PCIe-bound at
 * every frame size (pipck_rx_verify reads each packet in place with a wave of
 * its own: better for scattered packets, slower for small ones).  h_frames
 * pinned (pipck_host_alloc) for full rate; pageable works.  Synchronous;
 * *n_verified (optional) = frames with ok == PIPCK_RX_VERIFIED. */
int pipck_host_rx_verify_packed(pipck_ctx* ctx, const void* h_frames, const uint16_t* h_lens, uint64_t n_frames,
                                uint8_t* h_ok, uint64_t* n_verified);

/* ---- TX checksum fill of frames already in DEVICE memory ------------------
 * The TX mirror of pipck_rx_verify_device.  pip checksums every segment it
 * sends and stores htons(result) into the header: th_sum
 * (pip/protocol/pip_tcp_packet.cpp:124-134), uh_sum (pip/protocol/pip_udp.cpp:
 * 40-61), ip_sum (pip/pip_netif.cpp:80-97).  pipck_tx_fill_device does that for
 * n whole IP frames in the byte-packed layout of pipck_checksum_packed_bytes
 * (frame i of d_lens[i] bytes at d_arena + b_i, d_tile_off from
 * pipck_packed_bytes_index; link padding after the IP length allowed): it
 * parses each frame as pipck_rx_verify_device does, computes the IPv4 header
 * checksum and the TCP / UDP / ICMP / ICMPv6 checksum, and stores both fields
 * IN PLACE -- exactly the bytes pip's TX path writes.  d_done[i] receives
 *   PIPCK_TX_IP_FILLED   the IPv4 header checksum field (bytes 10-11) was written
 *   PIPCK_TX_L4_FILLED   the TCP / UDP / ICMP / ICMPv6 checksum field was written
 * A field is "taken as zero": its current bytes are ignored, so filling a frame
 * twice gives the same bytes.  No byte outside those two fields is ever written.
 * In full (tests/tx_reference.py restates these rules in plain integer
 * arithmetic and the kernel is held to it byte for byte):
 *   - Frames that are not written (d_done 0, no byte stored): a frame under 20
 *     bytes; a version that is neither 4 nor 6; IPv4 with IHL < 5, total length
 *     < header length, or total length > frame length; version 6 with fewer
 *     than 40 bytes, or with 40 + payload length > frame length.
 *   - IPv4 header: bytes 10-11 receive, big-endian, pip_ip_checksum
 *     (pip_checksum.cpp:35-39) of the whole header, options included (IHL
 *     5..15), with the field taken as zero; PIPCK_TX_IP_FILLED is set.  IPv6
 *     has no header checksum, so the bit stays clear.
 *   - An IPv4 fragment has MF or an offset set (ip_off & 0x3FFF != 0).  It gets
 *     the header field only.
 *   - The upper layer is located exactly as on RX.  IPv6 walks next headers 0,
 *     60 and 44 only, at most 8 of them.  Nothing more is written when a
 *     fragment header carries an offset or M (field & 0xFFF9), when a routing
 *     header (43) appears, when there is a ninth extension header, whatever it
 *     holds, or when an extension header does not fit in the payload.
 *   - The L4 length is the IP payload length from the upper-layer offset.  The
 *     UDP length field is not consulted.
 *   - The protocols are TCP (6), UDP (17), ICMP (1) over IPv4 only and ICMPv6
 *     (58) over IPv6 only.  Any other protocol (protocol 1 over IPv6 and 58
 *     over IPv4 included) gets nothing more.
 *   - An L4 length under 20 (TCP) or under 8 (UDP, ICMP, ICMPv6) gets nothing more.
 *   - The L4 field sits at message offset 16 (TCP), 6 (UDP) or 2 (ICMP,
 *     ICMPv6).  It receives, big-endian, pip_inet_checksum (IPv4) or
 *     pip_inet6_checksum (IPv6) of the message with the field taken as zero,
 *     over the frame's own addresses, protocol and L4 length
 *     (pip_checksum.cpp:42-87); ICMP over IPv4 has no pseudo-header and gets
 *     pip_ip_checksum of the message.  PIPCK_TX_L4_FILLED is set.
 *   - UDP over IPv4 is filled whatever the field held: there is no "zero means
 *     no checksum" rule on TX.
 *   - pip's values are stored as they are: a computed 0x0000 is stored as
 *     0x0000 (see the top of this header).  With PIPCK_TX_UDP_ZERO_AS_ONES in
 *     flags, a computed zero for UDP, over IPv4 or IPv6, is stored as 0xFFFF
 *     (RFC 768; RFC 8200 section 8.1).  An all-zero ICMP-over-IPv4 message
 *     (its field apart) gets pip's ~fold(0) = 0xFFFF.
 *   - Link padding after the IP length is not summed and not written.
 * Layout, alignment and index exactly as pipck_rx_verify_device: the arena
 * 128-byte aligned and readable to the 16-byte boundary after the last frame.
 * Bounded the same way: a tile of 64 frames whose bytes, as d_tile_off and
 * d_lens place them, reach past arena_bytes is neither read nor written, its
 * frames get d_done 0 and d_err (optional, device u32) gets
 * (1 << PIPCK_ERANGE).  PIPCK_EINVAL for a null pointer, an arena that is not
 * 128-byte aligned or unknown bits in flags; n_packets == 0 returns PIPCK_OK.
 * One kernel on `stream`, asynchronous, with no host-side allocation and no
 * host work (capturable in a graph): the byte-packed stream sums every frame
 * once, then a lane per frame parses its headers, derives both checksums from
 * that one sum and stores them.  The frames of one call must not be read or
 * written by other work on the device while it runs. */
#define PIPCK_TX_IP_FILLED 1u
#define PIPCK_TX_L4_FILLED 2u
#define PIPCK_TX_UDP_ZERO_AS_ONES 1u /* flags bit 0 */
int pipck_tx_fill_device(void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens, const uint64_t* d_tile_off,
                         uint64_t n_packets, uint32_t flags, uint8_t* d_done, uint32_t* d_err, void* stream);

/* The same fill for frames in the fixed-size slots of a TX ring in DEVICE
 * memory -- where a generator, a forwarder or a re-stamper writes frames whose
 * packed offsets it cannot know in advance.  Layout and arguments as
 * pipck_rx_verify_ring_n: frame i of d_lens[i] bytes (0..65,535) at d_arena +
 * i * slot_stride, the rest of each slot never read and never written; d_arena
 * 16-byte aligned, readable and writable for n_slots * slot_stride bytes;
 * slot_stride a multiple of 16 from 1,024 to 65,536.  For each frame the fields
 * written, their values, d_done[i] (PIPCK_TX_IP_FILLED, PIPCK_TX_L4_FILLED) and
 * the meaning of flags (PIPCK_TX_UDP_ZERO_AS_ONES) are those of
 * pipck_tx_fill_device for the same bytes: the rule list above is the one
 * definition.  Bounded on the device: a slot with d_lens[i] > slot_stride is
 * neither read nor written, gets d_done[i] = 0, and d_err (optional, device
 * u32) gets (1 << PIPCK_ERANGE).  PIPCK_EINVAL for a null d_arena, d_lens or
 * d_done, a misaligned arena, a stride outside the rule above or unknown bits
 * in flags; n_slots == 0 returns PIPCK_OK.  One kernel on `stream`,
 * asynchronous, with no host-side allocation and no per-ring state (capturable
 * in a graph; the schedule feedback of pipck_rx_verify_ring_n is not used):
 * blocks of 64 slots read only the frame bytes of their slots, then a lane per
 * slot parses the headers and stores each field with one aligned 16-bit store.
 * The slots of one call must not be read or written by other work on the
 * device while it runs. */
int pipck_tx_fill_ring(void* d_arena, uint64_t slot_stride, const uint16_t* d_lens, uint64_t n_slots,
                       uint32_t flags, uint8_t* d_done, uint32_t* d_err, void* stream);

/* ---- NAT and TTL rewrite of frames in a device ring ---------------------- */
/* A forwarder sends on a frame it has just verified with a few header fields
 * changed: the TTL or hop limit decremented (RFC 1812), addresses and ports
 * replaced (NAT, RFC 3022).  pipck_fwd_rewrite_ring does that for the frames of
 * a ring in DEVICE memory, from their headers alone: it stores the fields a
 * rule names and updates the IPv4 header checksum and the TCP / UDP / ICMPv6
 * checksum INCREMENTALLY (RFC 1624 eqn. 3) over the words of those fields.  So
 *   - the frame's one's-complement sums are preserved: a checksum that
 *     verified before the call verifies after it, and one that failed still
 *     fails -- a corrupted frame does not leave the box valid, as it would
 *     after rewriting the bytes and calling pipck_tx_fill_ring;
 *   - link padding and payload are never read: per frame the call reads the
 *     first min(length, 96) bytes (in aligned 16-byte chunks) and, only where
 *     an IPv6 extension chain carries the L4 fields past them, those headers;
 *   - with PIPCK_FWD_DEC_TTL the call is not idempotent: every call decrements.
 * Layout and host-side argument rules are those of pipck_tx_fill_ring: frame i
 * of d_lens[i] bytes at d_arena + i * slot_stride, d_arena 16-byte aligned,
 * slot_stride a multiple of 16 from 1,024 to 65,536, bytes of a slot past its
 * frame never read and never written.  d_rules is a table of n_rules rules,
 * 16-byte aligned; slot i takes rule d_rule_of ? d_rule_of[i] : 0.  d_done[i]
 * receives 0 or exactly one of PIPCK_FWD_DONE, PIPCK_FWD_EXPIRED,
 * PIPCK_FWD_UNHANDLED.  Per slot, in this order -- the first rule that applies
 * decides, and a frame is rewritten entirely or not at all
 * (tests/fwd_reference.py restates steps 2 to 6 in plain integer arithmetic and
 * the kernel is held to it byte for byte):
 *   1. Refusals, bounded on the device before any access they govern:
 *      d_lens[i] > slot_stride, or a rule index >= n_rules other than
 *      PIPCK_FWD_NO_RULE.  The slot is neither read nor written, d_done[i] = 0
 *      and d_err (optional, device u32) gets (1 << PIPCK_ERANGE); an index
 *      past the table never reads the table.  PIPCK_FWD_NO_RULE is not an
 *      error: the slot is neither read nor written, d_done[i] = 0, no error
 *      bit -- how a caller passes over frames that RX verification rejected.
 *   2. An invalid rule -- unknown ops bits, a family that is none of 0, 4, 6,
 *      or family 0 with PIPCK_FWD_SET_SRC or PIPCK_FWD_SET_DST: the frame is
 *      untouched, d_done[i] = 0, d_err gets (1 << PIPCK_EINVAL).
 *   3. A malformed frame, by the rules of pipck_tx_fill_device (under 20 bytes;
 *      a version that is neither 4 nor 6; IPv4 with IHL < 5, total length <
 *      header length or total length > frame length; version 6 under 40 bytes
 *      or with 40 + payload length > frame length): untouched, d_done[i] = 0,
 *      no error bit.
 *   4. PIPCK_FWD_DEC_TTL with a TTL (IPv4 byte 8) or hop limit (IPv6 byte 7)
 *      of 0 or 1: untouched, PIPCK_FWD_EXPIRED.  The host answers with ICMP.
 *   5. PIPCK_FWD_UNHANDLED, untouched, when
 *      - the rule's family is 4 or 6 and differs from the frame's version;
 *      - the rule sets an address or a port and the upper layer cannot be
 *        located -- it is located exactly as pipck_tx_fill_device locates it,
 *        so not for an IPv4 fragment (ip_off & 0x3FFF), an IPv6 fragment
 *        header with an offset or M, a routing header, a ninth extension
 *        header, or an extension header that does not fit in the payload;
 *      - the rule sets a port and the protocol is not TCP or UDP;
 *      - the rule sets an address and the protocol is none of TCP, UDP, ICMP
 *        over IPv4, ICMPv6 over IPv6;
 *      - the L4 length is under 20 (TCP) or under 8 (UDP, ICMP, ICMPv6).
 *      A rule with PIPCK_FWD_DEC_TTL alone never looks at the upper layer:
 *      fragments and any protocol are handled.
 *   6. Otherwise PIPCK_FWD_DONE.  Every field the rule names is stored:
 *      DEC_TTL stores the old value minus one; the source and destination
 *      address go to IPv4 bytes 12-15 and 16-19 (the first 4 bytes of src /
 *      dst) or IPv6 bytes 8-23 and 24-39; the ports to message offsets 0 and
 *      2.  Each checksum field that covers a named field is updated over
 *      exactly the 16-bit big-endian words of the named fields, whether or not
 *      their value changes:
 *          s   = (~HC & 0xFFFF) + sum(~old_k & 0xFFFF) + sum(new_k)    (exact)
 *          HC' = ~fold(s) & 0xFFFF     fold: end-around carry until s < 0x10000
 *      - The IPv4 header field (bytes 10-11): bytes 8-9 (TTL with protocol)
 *        for DEC_TTL, the address words for SET_SRC / SET_DST.  IPv6 has none.
 *      - The L4 field (message offset 16 for TCP, 6 for UDP, 2 for ICMPv6):
 *        the address words, through the pseudo-header, and for TCP and UDP the
 *        port words.  ICMP over IPv4 has no pseudo-header: its field is not
 *        touched.  A checksum field whose word list is empty is not touched.
 *      - UDP over IPv4 with a zero field keeps its zero (RFC 3022 section
 *        4.1); addresses and ports are still rewritten.  UDP over IPv6 with a
 *        zero field is updated like any value.
 *      - With PIPCK_FWD_UDP_ZERO_AS_ONES in flags, a UDP field that updates to
 *        0x0000 is stored as 0xFFFF, over IPv4 or IPv6.
 *      No byte outside the named fields and those two checksum fields changes
 *      value.  ICMP error payloads' embedded headers, the TCP / UDP length
 *      fields, SCTP and DCCP are not handled.
 * PIPCK_EINVAL (no launch) for a null d_arena, d_lens, d_done or d_rules,
 * n_rules == 0, a rule table or an arena that is not 16-byte aligned, a stride
 * outside the rule above or unknown bits in flags; n_slots == 0 returns
 * PIPCK_OK.  One kernel on `stream`, asynchronous, with no host-side
 * allocation and no per-ring state (capturable in a graph).  The slots of one
 * call must not be read or written by other work on the device while it runs. */
#define PIPCK_FWD_SET_SRC   1u   /* ops bits */
#define PIPCK_FWD_SET_DST   2u
#define PIPCK_FWD_SET_SPORT 4u
#define PIPCK_FWD_SET_DPORT 8u
#define PIPCK_FWD_DEC_TTL   16u
#define PIPCK_FWD_UDP_ZERO_AS_ONES 1u   /* flags bit 0 */
#define PIPCK_FWD_DONE      1u   /* d_done values, exclusive */
#define PIPCK_FWD_EXPIRED   2u
#define PIPCK_FWD_UNHANDLED 4u
#define PIPCK_FWD_NO_RULE   0xFFFFFFFFu

typedef struct pipck_fwd_rule {   /* 48 bytes, 16-byte aligned table */
    uint32_t ops;        /* PIPCK_FWD_SET_* | PIPCK_FWD_DEC_TTL */
    uint8_t  family;     /* 4 or 6: the frames it applies to; 0 = either, only without SET_SRC/SET_DST */
    uint8_t  pad[3];
    uint8_t  src[16];    /* wire bytes; IPv4 uses the first 4 */
    uint8_t  dst[16];
    uint8_t  sport[2];   /* wire bytes */
    uint8_t  dport[2];
    uint8_t  pad2[4];
} pipck_fwd_rule;

int pipck_fwd_rewrite_ring(void* d_arena, uint64_t slot_stride, const uint16_t* d_lens, uint64_t n_slots,
                           const pipck_fwd_rule* d_rules, uint32_t n_rules, const uint32_t* d_rule_of,
                           uint32_t flags, uint8_t* d_done, uint32_t* d_err, void* stream);

/* The same rewrite for a byte-packed batch in DEVICE memory -- what
 * pipck_rx_verify_device has just verified and pipck_host_rx_verify_packed
 * uploads: capture buffers and socket rings read in order.  Layout, alignment
 * and index are exactly those of pipck_rx_verify_device and
 * pipck_tx_fill_device: frame i of d_lens[i] bytes (0..65,535) at d_arena + b_i,
 * d_tile_off from pipck_packed_bytes_index, the arena 128-byte aligned, readable
 * and writable to the 16-byte boundary after the last frame.  The rule table,
 * d_rule_of, flags, the d_done values and PIPCK_FWD_NO_RULE are exactly those of
 * pipck_fwd_rewrite_ring.  Decisions, in this order:
 *   - First the tile bound of pipck_tx_fill_device: a tile of 64 frames whose
 *     bytes, as d_tile_off and d_lens place them, reach past arena_bytes is
 *     neither read nor written, its frames get d_done 0 and d_err (optional,
 *     device u32) gets (1 << PIPCK_ERANGE).  Its rules are not consulted: an
 *     invalid rule there sets no PIPCK_EINVAL bit.
 *   - Then, per frame, steps 1 to 6 of pipck_fwd_rewrite_ring's list above,
 *     which stays the one definition; only the refusal d_lens[i] > slot_stride
 *     drops out, there being no stride.
 * Reads: per frame only the aligned 16-byte chunks that hold its first
 * min(length, 96) bytes, never a chunk past the one holding its last byte, and,
 * only where an IPv6 extension chain carries the L4 fields past them, those
 * headers, from the frame's own bytes.  Payload and link padding are never read.
 * Stores: every store instruction covers only bytes of its own frame -- the
 * named fields, the byte beside the TTL or hop limit (bytes 8-9 of IPv4, 6-7 of
 * IPv6 are stored together, as the ring call stores them) and the two checksum
 * fields.  No store spans into another frame and none is a read-modify-write of
 * a wider unit: a frame that starts at a multiple of 4 gets aligned 32- and
 * 16-bit stores, one at 2 mod 4 16-bit stores, one at an odd address single
 * bytes, so the neighbouring frame's bytes in the same dword may be stored by
 * another lane, wave or block at the same time.  The frames of one call must
 * not be read or written by other work on the device while it runs.
 * PIPCK_EINVAL (no launch) for unknown bits in flags (checked first), then for a
 * null d_arena, d_lens, d_tile_off, d_done or d_rules, n_rules == 0, a rule
 * table that is not 16-byte aligned or an arena that is not 128-byte aligned;
 * n_packets == 0 returns PIPCK_OK.  One kernel on `stream`, asynchronous, with
 * no host-side allocation and no per-call state (capturable in a graph).
 * Cost on one MI355X: 59-93 ps a frame where frames
 * start 4-aligned, on 8,920-8,940-byte frames 0.07 of pipck_rx_verify_device's
 * time; 141-162 ps where they start at every residue and go out byte by byte. */
int pipck_fwd_rewrite_device(void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens,
                             const uint64_t* d_tile_off, uint64_t n_packets, const pipck_fwd_rule* d_rules,
                             uint32_t n_rules, const uint32_t* d_rule_of, uint32_t flags, uint8_t* d_done,
                             uint32_t* d_err, void* stream);

/* ---- flow classification: d_rule_of from the frames themselves ------------ */
/* The rewrite calls take one rule index per frame.  pipck_fwd_classify_ring and
 * pipck_fwd_classify_device produce it on the device: per frame they parse the
 * headers, look the frame's 5-tuple up in a binding table in DEVICE memory and
 * write d_rule_of -- so verify -> classify -> rewrite can be enqueued on one
 * stream, or captured in one graph, with no host work in between.
 *
 * Key.  A frame has a key when it is well-formed (step 3 of
 * pipck_fwd_rewrite_ring's list), its upper layer is located exactly as
 * pipck_tx_fill_device locates it (not for an IPv4 fragment, an IPv6 fragment
 * header with an offset or M, a routing header, a ninth extension header or an
 * extension header that does not fit in the payload), its protocol is TCP, UDP,
 * ICMP over IPv4 or ICMPv6 over IPv6 and its L4 length is at least 20 (TCP) or 8
 * (the others): exactly the frames an address-and-port rule of their family
 * rewrites or finds expired.  The key is then the family, the protocol, the two
 * addresses as wire bytes (IPv4: the first 4 bytes, the other 12 zero) and, for
 * TCP and UDP, the four port bytes at message offset 0 (zero for ICMP / ICMPv6).
 *
 * Hash, in plain integer arithmetic modulo 2^32, so any binding can build a
 * table: read the key's 40 bytes as ten little-endian u32 k[0..9]; start with
 * x = 0; for each k[j] in order  x = rotl32(x ^ k[j], 13) * 0x9E3779B1;  then
 * x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13.  The all-zero key hashes to
 * 0x00000000; {src 10.0.0.1, dst 10.0.0.2, sport 1234, dport 80, proto 6,
 * family 4} hashes to 0x1C838748.
 *
 * Table.  n_slots entries of 48 bytes, n_slots a power of two up to 2^31,
 * 16-byte aligned in device memory.  An entry with tag 0 is empty; an occupied
 * one has tag = pipck_fwd_key_hash(key) | 0x80000000.  Lookup, for
 * p = 0 .. PIPCK_FWD_MAX_PROBE - 1, looks at entry (hash + p) & (n_slots - 1):
 * a tag of 0 ends the search as a miss; a tag equal to hash | 0x80000000
 * together with all 40 key bytes equal is a hit; after 64 probes the search
 * ends as a miss.  The loop is bounded whatever the table holds and every index
 * is masked, so a corrupt or foreign table can give wrong rules but never a
 * read outside n_slots entries and never an unbounded loop.  `rule` is not
 * bounded here: the rewrite call bounds it against its own n_rules.
 * Keep the load at or below 0.5: linear probing with this hash, measured on a
 * CPU over sequential-port IPv4 bindings, random IPv6 bindings and one host's
 * DNS-style bindings, had a longest probe of 14-26 at 4 K slots, 22-23 at 64 K
 * and 37-45 at 1 M slots at load 0.5 (8-9 at 64 K slots and load 0.25), but
 * 120-132 at 64 K slots and load 0.75 -- past the bound of 64. */
typedef struct pipck_fwd_key {   /* 40 bytes */
    uint8_t src[16];   /* wire bytes; IPv4 uses the first 4, the other 12 are zero */
    uint8_t dst[16];
    uint8_t sport[2];  /* wire bytes; zero for ICMP and ICMPv6 */
    uint8_t dport[2];
    uint8_t proto;     /* 6, 17, 1 (IPv4 only), 58 (IPv6 only) */
    uint8_t family;    /* 4 or 6 */
    uint8_t pad[2];    /* zero */
} pipck_fwd_key;
typedef struct pipck_fwd_entry { /* 48 bytes: three 16-byte chunks, like pipck_fwd_rule */
    pipck_fwd_key key;
    uint32_t rule;     /* what d_rule_of receives on a hit; may be PIPCK_FWD_NO_RULE */
    uint32_t tag;      /* 0 = empty; else pipck_fwd_key_hash(key) | 0x80000000 */
} pipck_fwd_entry;
#define PIPCK_FWD_MAX_PROBE    64u
#define PIPCK_FWD_CLASS_HIT     1u   /* d_class values, exclusive; 0 = malformed or refused */
#define PIPCK_FWD_CLASS_MISS    2u
#define PIPCK_FWD_CLASS_UNKEYED 4u
#define PIPCK_FWD_CLASS_PASSED  8u

/* Host functions: pure CPU, no device, usable without a GPU.
 * pipck_fwd_key_hash: the hash above (0 for a null key).
 * pipck_fwd_table_build zeroes table[0, n_slots), then inserts the keys in
 * order, key i with rules[i], each at the first empty entry of its probe
 * sequence.  PIPCK_EINVAL for a null table, null keys or rules with n_keys > 0,
 * n_slots zero, not a power of two or above 2^31, a key with nonzero pad, a
 * family that is neither 4 nor 6, family 4 with a nonzero address byte 4..15, a
 * protocol outside {6, 17, 1 with family 4, 58 with family 6}, nonzero ports
 * with ICMP / ICMPv6, or a duplicate key; PIPCK_ERANGE when a key finds no empty
 * entry within 64 probes.  On success the table is fully determined by this
 * rule (byte-comparable with any other implementation of it); on failure its
 * contents are unspecified.  The caller uploads it to a 16-byte-aligned device
 * buffer.
 * pipck_fwd_frame_key returns 1 and writes *key when the frame of len bytes has
 * a key by the rules above, and 0 when it has none or an argument is null; it
 * reads nothing past len.  This is how a host turns a frame reported as
 * PIPCK_FWD_CLASS_MISS into a new binding. */
uint32_t pipck_fwd_key_hash(const pipck_fwd_key* key);
int pipck_fwd_table_build(const pipck_fwd_key* keys, const uint32_t* rules, uint64_t n_keys, pipck_fwd_entry* table,
                          uint64_t n_slots);
int pipck_fwd_frame_key(const void* frame, uint32_t len, pipck_fwd_key* key);

/* The device calls.  Layouts and host-side argument rules are those of
 * pipck_fwd_rewrite_ring and pipck_fwd_rewrite_device respectively; the arena
 * is const: NO byte of it is ever written.  d_rule_of[i] (u32, required)
 * receives the frame's rule index, d_class[i] (u8, optional) one of the
 * PIPCK_FWD_CLASS_* values or 0.  d_ok (optional) holds the PIPCK_RX_* verdicts
 * of the same frames.  Per frame, the first rule that applies decides:
 *   1. Layout refusal -- ring: d_lens[i] > slot_stride; byte-packed: the tile
 *      bound of pipck_tx_fill_device, for all frames of the tile.  The frame is
 *      not read, d_rule_of[i] = PIPCK_FWD_NO_RULE, class 0, d_err (optional,
 *      device u32) gets (1 << PIPCK_ERANGE).
 *   2. Verdict gate, when d_ok is given and (d_ok[i] & ok_mask) != ok_mask: the
 *      frame is not read, PIPCK_FWD_NO_RULE, class PIPCK_FWD_CLASS_PASSED, no
 *      error bit.  ok_mask = 3 lets verified and unchecked frames through,
 *      ok_mask = 7 only verified ones, ok_mask = 0 every frame.
 *   3. A malformed frame (step 3 of pipck_fwd_rewrite_ring's list):
 *      PIPCK_FWD_NO_RULE, class 0, no error bit.
 *   4. A well-formed frame without a key (above): other_rule, class
 *      PIPCK_FWD_CLASS_UNKEYED.  A router gives these its DEC_TTL-only rule.
 *   5. A keyed frame is looked up: a hit gives the entry's rule and class
 *      PIPCK_FWD_CLASS_HIT, a miss miss_rule and class PIPCK_FWD_CLASS_MISS.
 * miss_rule and other_rule may be any u32, PIPCK_FWD_NO_RULE included.
 * Reads are exactly those of the rewrite calls: the aligned 16-byte chunks
 * holding a frame's first min(length, 96) bytes, never a chunk past the one
 * holding its last byte, and the frame's own bytes only where an IPv6 extension
 * chain carries the ports past them; a gated or refused frame loads nothing.
 * Of the table a probe that does not match reads 16 bytes, a hit 48.  d_rule_of
 * and d_class are never written outside [0, n).
 * PIPCK_EINVAL (no launch) for an ok_mask above 7 (checked first), then, unless
 * the frame count is 0 (PIPCK_OK), for a null d_arena, d_lens, d_table,
 * d_rule_of or (byte-packed) d_tile_off, n_slots zero, not a power of two or
 * above 2^31, a table that is not 16-byte aligned, and the layout's own
 * alignment and stride rules.  One kernel on `stream`, asynchronous, with no
 * allocation and no per-call state (capturable in a graph).
 * Cost on one MI355X, every frame a hit in a table of
 * 65,536 slots at load 0.5: 39-59 ps a frame, 0.57-0.72 of the rewrite call's
 * time on the same frames, about a third of it table probes; on 8,920-8,940-byte
 * frames 0.035 (ring) and 0.045 (byte-packed) of the RX verifier's time. */
int pipck_fwd_classify_ring(const void* d_arena, uint64_t slot_stride, const uint16_t* d_lens, uint64_t n_slots_ring,
                            const pipck_fwd_entry* d_table, uint64_t n_slots, uint32_t miss_rule, uint32_t other_rule,
                            const uint8_t* d_ok, uint32_t ok_mask, uint32_t* d_rule_of, uint8_t* d_class,
                            uint32_t* d_err, void* stream);
int pipck_fwd_classify_device(const void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens,
                              const uint64_t* d_tile_off, uint64_t n_packets, const pipck_fwd_entry* d_table,
                              uint64_t n_slots, uint32_t miss_rule, uint32_t other_rule, const uint8_t* d_ok,
                              uint32_t ok_mask, uint32_t* d_rule_of, uint8_t* d_class, uint32_t* d_err, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIPCK_H */

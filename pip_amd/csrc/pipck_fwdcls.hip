// pipck_fwdcls.hip -- flow classification for the NAT rewrite calls
// (pipck_fwd_classify_ring, pipck_fwd_classify_device, include/pipck.h): per
// frame the kernel loads the first 96 bytes as the rewrite kernels do, builds the
// frame's 5-tuple key, looks it up in a binding table in device memory and
// writes the frame's rule index, which pipck_fwd_rewrite_* then takes as
// d_rule_of.  The arena is read-only here: no store of this file goes to it.
// The payload is never read, so the traffic is set by header lines, not frame
// bytes.  The host functions of the table live here too.
//
// A file of its own, with a parse of its own (pipck_fwdkey.hpp, which calls
// nothing of the RX, TX and forwarding parse headers): every other kernel of the
// library compiles to exactly the code it had.
#include "pipck_common.hpp"
#include "pipck_device.hpp"
#include "pipck_fwdkey.hpp"

namespace pipck {

constexpr uint32_t kClsB = 256;    // frames per block: 64 per wave, the four waves independent of each other
constexpr int kClsWords = 24;      // the window: 96 bytes from the frame's start
constexpr uint32_t kClsWinMin = 80;  // what the six chunks hold of a frame at any start (96 - 15, down to a dword)
constexpr uint32_t kClsNoRule = PIPCK_FWD_NO_RULE;
static_assert(sizeof(pipck_fwd_entry) == 48 && alignof(pipck_fwd_entry) <= 16, "pipck_fwd_entry is three 16-byte chunks");

// The window as fwdkey_parse asks for it: frame bytes [j, j + 4), j a multiple of
// 4, from the registers where they hold them all, else from the frame's own
// bytes one at a time (p may have any alignment; the parse has bounded j + 4 by
// the frame's length).  A run-time j takes a select chain: an indexed copy would
// go through scratch memory.  win >= kClsWinMin, so a constant j below that
// folds to the register itself.
struct ClsWords {
    const uint8_t* p;
    const uint32_t (&a)[kClsWords];
    uint32_t win;
    __device__ __forceinline__ uint32_t operator()(uint32_t j) const {
        if (j + 4u <= kClsWinMin || j + 4u <= win) {
            uint32_t x = 0;
#pragma unroll
            for (int i = 0; i < kClsWords; i++)
                if ((uint32_t)i == j >> 2) x = a[i];
            return x;
        }
        return (uint32_t)p[j] | (uint32_t)p[j + 1] << 8 | (uint32_t)p[j + 2] << 16 | (uint32_t)p[j + 3] << 24;
    }
};

// The table as fwdkey_lookup asks for it: one 16-byte load per chunk.  i is
// masked by the caller, so 3 i + c lies inside the table's 3 n_slots chunks.
struct ClsTable {
    const u32x4* t;
    __device__ __forceinline__ FwdChunk operator()(uint32_t i, uint32_t c) const {
        const u32x4 q = load_plain(t + 3ull * i + c);
        return FwdChunk{q.x, q.y, q.z, q.w};
    }
};

// What becomes of one frame that is read: its rule index and class.
struct ClsOut {
    uint32_t rule, cls;
};
__device__ __forceinline__ ClsOut cls_frame(const ClsWords& w, uint32_t len, const u32x4* table, uint32_t mask,
                                            uint32_t miss_rule, uint32_t other_rule) {
    uint32_t k[kFwdKeyWords];
    const uint32_t kind = fwdkey_parse(w, len, k);
    if (kind == kFwdKeyMalformed) return ClsOut{kClsNoRule, 0u};
    if (kind == kFwdKeyNone) return ClsOut{other_rule, PIPCK_FWD_CLASS_UNKEYED};
    uint32_t rule = 0;
    if (fwdkey_lookup(ClsTable{table}, mask, k, fwdkey_hash(k), rule)) return ClsOut{rule, PIPCK_FWD_CLASS_HIT};
    return ClsOut{miss_rule, PIPCK_FWD_CLASS_MISS};
}

// Result stores: range-checked against the wave's own elements, with the
// write-through policy of store_result8 (pipck_device.hpp).
__device__ __forceinline__ void store_result32(buf_t r, uint32_t byte_off, uint32_t v) {
    __builtin_amdgcn_raw_buffer_store_b32(v, r, (int)byte_off, 0, kStoreSc1);
}
__device__ __forceinline__ void cls_store(uint32_t* rule_of, uint8_t* cls, uint64_t s0, uint32_t nw, uint32_t lane,
                                          const ClsOut& o) {
    store_result32(buf_rsrc(rule_of + s0, 4u * nw), 4u * lane, o.rule);
    if (cls) store_result8(buf_rsrc(cls + s0, nw), lane, o.cls);
}

// k_fwd_ring's front end (pipck_fwd.hip): a wave takes 64 slots, lane g slot g;
// eight lanes per slot load its six aligned chunks, chunk c iff 16 c < Lw, through
// the wave's own 6 x 65 x 16 bytes of LDS; no block barrier.  Lw = min(length,
// 96), and 0 -- nothing loaded -- for a slot whose length passes the stride
// (refused), one the verdict gate passes over and a lane past the ring's end.
__global__ __launch_bounds__(256) void k_fwd_classify_ring(const uint8_t* __restrict__ arena, uint32_t stride,
                                                           const uint16_t* __restrict__ lens, uint64_t n,
                                                           const u32x4* __restrict__ table, uint32_t mask,
                                                           uint32_t miss_rule, uint32_t other_rule,
                                                           const uint8_t* __restrict__ ok, uint32_t ok_mask,
                                                           uint32_t* __restrict__ rule_of, uint8_t* __restrict__ cls,
                                                           uint32_t* __restrict__ err) {
    __shared__ u32x4 hdr[kClsB / 64][6][65];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t s0 = (uint64_t)blockIdx.x * kClsB + 64u * w;  // the wave's first slot
    if (s0 >= n) return;
    const uint32_t nw = (uint32_t)min<uint64_t>(64, n - s0);
    const bool valid = lane < nw;
    const uint32_t L = valid ? (uint32_t)lens[s0 + lane] : 0u;
    const bool bad = valid && L > stride;  // bounded before any access
    const bool gated = valid && !bad && ok && ((uint32_t)ok[s0 + lane] & ok_mask) != ok_mask;
    const bool go = valid && !bad && !gated;
    const uint32_t Lw = go ? min(L, 4u * kClsWords) : 0u;

    const buf_t rb = buf_rsrc(arena + s0 * stride, nw * stride);  // the wave's slots
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
    uint32_t a[kClsWords];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const u32x4 x = hdr[w][k][lane];
        a[4 * k] = x.x, a[4 * k + 1] = x.y, a[4 * k + 2] = x.z, a[4 * k + 3] = x.w;
    }

    ClsOut o{kClsNoRule, gated ? PIPCK_FWD_CLASS_PASSED : 0u};
    if (go) o = cls_frame(ClsWords{arena + (s0 + lane) * stride, a, 4u * kClsWords}, L, table, mask, miss_rule, other_rule);
    refuse(err, bad);
    cls_store(rule_of, cls, s0, nw, lane, o);
}

// k_fwd_device's front end (pipck_fwddev.hip): a wave takes one tile of 64
// frames, lane g frame g; the starts from the wave scan of the lengths, the tile
// bound scalar and overflow-safe before anything of the tile is read, six chunks
// per frame (chunk c iff 16 c < h + Lw, h = start & 15), realigned by h with
// static register indices.  The parse is told win = (96 - h) & ~3, the bytes the
// six chunks are sure to hold; past them it reads the frame's own bytes.
__global__ __launch_bounds__(256) void k_fwd_classify_device(const uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                             const uint16_t* __restrict__ lens,
                                                             const uint64_t* __restrict__ tile_off, uint64_t n,
                                                             const u32x4* __restrict__ table, uint32_t mask,
                                                             uint32_t miss_rule, uint32_t other_rule,
                                                             const uint8_t* __restrict__ ok, uint32_t ok_mask,
                                                             uint32_t* __restrict__ rule_of, uint8_t* __restrict__ cls,
                                                             uint32_t* __restrict__ err) {
    __shared__ u32x4 hdr[kClsB / 64][6][65];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t tile = (uint64_t)blockIdx.x * (kClsB / 64) + w;
    const uint64_t s0 = tile * 64;  // the wave's first frame
    if (s0 >= n) return;
    const uint32_t nw = (uint32_t)min<uint64_t>(64, n - s0);
    const bool valid = lane < nw;
    const uint32_t L = valid ? (uint32_t)lens[s0 + lane] : 0u;

    const uint32_t incl = wave_incl_scan(L);
    const uint64_t toff = first_lane_u64(tile_off[tile]);
    const uint32_t tile_len = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (!(toff <= arena_bytes && (uint64_t)tile_len <= arena_bytes - toff)) {  // wave-uniform
        refuse(err, lane == 0);
        cls_store(rule_of, cls, s0, nw, lane, ClsOut{kClsNoRule, 0u});
        return;
    }
    const uint64_t first = (uint64_t)(uintptr_t)arena + toff;
    const uint64_t base = first & ~15ull;  // the chunk holding the tile's first byte
    const uint32_t lead = (uint32_t)(first - base);
    const uint32_t start = lead + incl - L;  // relative to base
    const uint32_t h = start & 15u;

    const bool gated = valid && ok && ((uint32_t)ok[s0 + lane] & ok_mask) != ok_mask;
    const bool go = valid && !gated;
    const uint32_t Lw = go ? min(L, 4u * kClsWords) : 0u;

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
    uint32_t u[kClsWords + 3], a[kClsWords];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const u32x4 x = hdr[w][k][lane];
        u[4 * k] = x.x, u[4 * k + 1] = x.y, u[4 * k + 2] = x.z, u[4 * k + 3] = x.w;
    }
    u[24] = u[25] = u[26] = 0u;
#pragma unroll
    for (int k = 0; k < kClsWords + 1; k++) u[k] = u[k] ^ ((u[k] ^ u[k + 2]) & m2);
#pragma unroll
    for (int k = 0; k < kClsWords + 1; k++) u[k] = u[k] ^ ((u[k] ^ u[k + 1]) & m1);
#pragma unroll
    for (int k = 0; k < kClsWords; k++) a[k] = __builtin_amdgcn_alignbyte(u[k + 1], u[k], r8);

    ClsOut o{kClsNoRule, gated ? PIPCK_FWD_CLASS_PASSED : 0u};
    if (go)
        o = cls_frame(ClsWords{reinterpret_cast<const uint8_t*>(base) + start, a, (4u * kClsWords - h) & ~3u}, L, table,
                      mask, miss_rule, other_rule);
    cls_store(rule_of, cls, s0, nw, lane, o);
}

// The arguments both calls share; `fn` names the call in the error text.
static int cls_common_args(const char* fn, const pipck_fwd_entry* d_table, uint64_t n_slots, const uint32_t* d_rule_of) {
    if (!d_table || !d_rule_of) {
        set_error(std::string(fn) + ": null pointer");
        return PIPCK_EINVAL;
    }
    if (!fwdkey_table_slots_valid(n_slots) || (uintptr_t)d_table % 16) {
        set_error(std::string(fn) + ": the binding table must be 16-byte aligned and hold a power of two of entries, "
                                    "from 1 to 2^31");
        return PIPCK_EINVAL;
    }
    return PIPCK_OK;
}

// pipck_fwd_classify_ring: pipck_fwd_rewrite_ring's argument rules plus the
// table's, then one k_fwd_classify_ring over blocks of 256 slots -- nothing
// allocated, nothing remembered, so the call can be captured
static int launch_ring_cls(const void* d_arena, uint64_t stride, const uint16_t* d_lens, uint64_t n,
                           const pipck_fwd_entry* d_table, uint64_t n_slots, uint32_t miss_rule, uint32_t other_rule,
                           const uint8_t* d_ok, uint32_t ok_mask, uint32_t* d_rule_of, uint8_t* d_class,
                           uint32_t* d_err, hipStream_t s) {
    static const char fn[] = "pipck_fwd_classify_ring";
    if (ok_mask > 7u) {
        set_error(std::string(fn) + ": ok_mask above 7");
        return PIPCK_EINVAL;
    }
    if (n == 0) return PIPCK_OK;
    if (!d_arena || !d_lens) {
        set_error(std::string(fn) + ": null pointer");
        return PIPCK_EINVAL;
    }
    if (const int rc = cls_common_args(fn, d_table, n_slots, d_rule_of)) return rc;
    if ((uintptr_t)d_arena % 16 || stride % 16 || stride < 1024 || stride > 65536) {
        set_error(std::string(fn) + ": the arena must be 16-byte aligned and the slot stride a multiple of 16 bytes "
                                    "from 1 KiB to 64 KiB");
        return PIPCK_EINVAL;
    }
    const uint64_t blocks = (n + kClsB - 1) / kClsB;
    if (blocks > 0x7FFFFFFFull) {
        set_error(std::string(fn) + ": too many slots for one launch");
        return PIPCK_ERANGE;
    }
    PIPCK_LAUNCH(k_fwd_classify_ring, dim3((uint32_t)blocks), dim3(256), 0, s, (const uint8_t*)d_arena,
                 (uint32_t)stride, d_lens, n, (const u32x4*)d_table, (uint32_t)(n_slots - 1), miss_rule, other_rule,
                 d_ok, ok_mask, d_rule_of, d_class, d_err);
    PIPCK_LAUNCHED("k_fwd_classify_ring");
    return PIPCK_OK;
}

// pipck_fwd_classify_device: the byte-packed calls' argument rules plus the
// table's, then one k_fwd_classify_device over blocks of four tiles
static int launch_packedb_cls(const void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens,
                              const uint64_t* d_tile_off, uint64_t n, const pipck_fwd_entry* d_table, uint64_t n_slots,
                              uint32_t miss_rule, uint32_t other_rule, const uint8_t* d_ok, uint32_t ok_mask,
                              uint32_t* d_rule_of, uint8_t* d_class, uint32_t* d_err, hipStream_t s) {
    static const char fn[] = "pipck_fwd_classify_device";
    if (ok_mask > 7u) {
        set_error(std::string(fn) + ": ok_mask above 7");
        return PIPCK_EINVAL;
    }
    if (n == 0) return PIPCK_OK;
    if (!d_arena || !d_lens || !d_tile_off) {
        set_error(std::string(fn) + ": null pointer");
        return PIPCK_EINVAL;
    }
    if (const int rc = cls_common_args(fn, d_table, n_slots, d_rule_of)) return rc;
    if ((uintptr_t)d_arena % 128) {
        set_error(std::string(fn) + ": the arena must be 128-byte aligned");
        return PIPCK_EINVAL;
    }
    const uint64_t tiles = (n + 63) / 64;
    if (tiles > 0x7FFFFFFFull) {
        set_error(std::string(fn) + ": more than 2^37 packets in one launch");
        return PIPCK_ERANGE;
    }
    const uint64_t blocks = (tiles + kClsB / 64 - 1) / (kClsB / 64);
    PIPCK_LAUNCH(k_fwd_classify_device, dim3((uint32_t)blocks), dim3(256), 0, s, (const uint8_t*)d_arena, arena_bytes,
                 d_lens, d_tile_off, n, (const u32x4*)d_table, (uint32_t)(n_slots - 1), miss_rule, other_rule, d_ok,
                 ok_mask, d_rule_of, d_class, d_err);
    PIPCK_LAUNCHED("k_fwd_classify_device");
    return PIPCK_OK;
}

}  // namespace pipck

extern "C" {

uint32_t pipck_fwd_key_hash(const pipck_fwd_key* key) {
    if (!key) return 0;
    uint32_t k[pipck::kFwdKeyWords];
    pipck::fwdkey_words(*key, k);
    return pipck::fwdkey_hash(k);
}

int pipck_fwd_table_build(const pipck_fwd_key* keys, const uint32_t* rules, uint64_t n_keys, pipck_fwd_entry* table,
                          uint64_t n_slots) {
    const int rc = pipck::fwdkey_table_build(keys, rules, n_keys, table, n_slots);
    if (rc == PIPCK_EINVAL)
        pipck::set_error("pipck_fwd_table_build: a null pointer, a slot count that is no power of two from 1 to 2^31, "
                         "an invalid key or a duplicate key");
    if (rc == PIPCK_ERANGE) pipck::set_error("pipck_fwd_table_build: no empty entry within 64 probes");
    return rc;
}

int pipck_fwd_frame_key(const void* frame, uint32_t len, pipck_fwd_key* key) {
    if (!frame || !key) return 0;
    uint32_t k[pipck::kFwdKeyWords];
    if (pipck::fwdkey_of_frame(static_cast<const uint8_t*>(frame), len, k) != pipck::kFwdKeyed) return 0;
    pipck::fwdkey_from_words(k, *key);
    return 1;
}

int pipck_fwd_classify_ring(const void* d_arena, uint64_t slot_stride, const uint16_t* d_lens, uint64_t n_slots_ring,
                            const pipck_fwd_entry* d_table, uint64_t n_slots, uint32_t miss_rule, uint32_t other_rule,
                            const uint8_t* d_ok, uint32_t ok_mask, uint32_t* d_rule_of, uint8_t* d_class,
                            uint32_t* d_err, void* stream) {
    return pipck::launch_ring_cls(d_arena, slot_stride, d_lens, n_slots_ring, d_table, n_slots, miss_rule, other_rule,
                                  d_ok, ok_mask, d_rule_of, d_class, d_err, pipck::as_stream(stream));
}

int pipck_fwd_classify_device(const void* d_arena, uint64_t arena_bytes, const uint16_t* d_lens,
                              const uint64_t* d_tile_off, uint64_t n_packets, const pipck_fwd_entry* d_table,
                              uint64_t n_slots, uint32_t miss_rule, uint32_t other_rule, const uint8_t* d_ok,
                              uint32_t ok_mask, uint32_t* d_rule_of, uint8_t* d_class, uint32_t* d_err, void* stream) {
    return pipck::launch_packedb_cls(d_arena, arena_bytes, d_lens, d_tile_off, n_packets, d_table, n_slots, miss_rule,
                                     other_rule, d_ok, ok_mask, d_rule_of, d_class, d_err, pipck::as_stream(stream));
}

}  // extern "C"

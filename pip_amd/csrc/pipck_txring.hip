// pipck_txring.hip -- TX checksum fill of IP frames in the fixed-size slots of a
// ring in device memory (pipck_tx_fill_ring, include/pipck.h).  The TX mirror of
// k_ring (pipck_rxdev.hip): the same slot-group streams (pipck_ring.hpp) leave
// each slot's frame sum and header window in the block's LDS, and where k_ring
// judges a slot with rx_from_window, k_ring_tx fills it with tx_from_window
// (pipck_txparse.hpp) -- the rules of pipck_tx_fill_device, one definition.
//
// A file of its own: pipck_txparse.hpp calls the plain inline helpers of
// pipck_rxparse.hpp, and a second caller in pipck_rxdev.hip changes how the
// compiler inlines them into the RX ring kernels (a few instructions of every
// k_ring body moved when k_ring_tx stood beside them).  From here the RX
// kernels compile to exactly the code they had.
#include "pipck_common.hpp"
#include "pipck_ring.hpp"
#include "pipck_txparse.hpp"

namespace pipck {

// k_ring's prologue and streams as they are (the 64 lengths, bad = L > stride,
// ring_short for frames up to 32 chunks, else ring_rows on each wave's own 16
// slots or dealt round-robin from T >= kRingCoopRows * nb), the interleaved
// stream over all 64 slots at once (G = 64).  Of the tune word it reads only
// kRingOwnSlots and kRingAllCoop of ring_mode, so a test can force either row
// stream on any data; the wave arm, the alt-schedule bit, loads, blocks and the
// adapt bits are ignored: one instantiation, <8, 12>, no feedback, no per-ring
// state.  62 VGPRs, no scratch, 8 waves per SIMD -- k_ring<8, 12>'s occupancy,
// which the sparse and short rings need.
//
// After the block's barrier wave 0 takes slot g in lane g: the window as k_ring
// builds it, tx_from_window on the slot's frame sum, and, once both of a lane's
// values are known, its stores.
//
// Why one 16-bit store per field is always right.  A slot starts at a multiple
// of 16 (the arena is 16-byte aligned, the stride a multiple of 16).  The IPv4
// field is at 10.  The L4 field is at l4off + 16 (TCP), + 6 (UDP) or + 2 (ICMP,
// ICMPv6), and l4off is IHL * 4 or 40 + 8k: a multiple of 4.  So every field
// offset is even -- an aligned halfword -- and, being even and at most 14 mod
// 16, its two bytes lie in one 16-byte chunk, hence in one 128-byte line.
// The stores go through the resource of the block's own slots (nb * stride
// bytes), at g * stride + 10 and g * stride + l4_at; tx_from_window gives a
// field only where it lies inside the frame, so inside the slot.  No other
// block ever loads a byte of these slots: the byte-packed kernel's ordering
// argument (tiles sharing a line) has nothing to order
// here.  Lanes past nb and refused slots hold done = 0 and store no field.
template <int U, int UD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void k_ring_tx(
    uint8_t* arena, uint32_t stride, const uint16_t* __restrict__ lens, uint64_t n, uint32_t flags,
    uint8_t* __restrict__ done, uint32_t* __restrict__ err, uint32_t kflags) {
    constexpr uint32_t B = kRingB;
    __shared__ RingLds t;
    const int lane = threadIdx.x & 63;
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t b0 = (uint64_t)blockIdx.x * B;  // the block's first slot
    const uint32_t nb = (uint32_t)min<uint64_t>(B, n - b0);
    const bool valid = (uint32_t)lane < nb;
    const uint32_t L = valid ? (uint32_t)lens[b0 + lane] : 0u;  // every wave: all 64 lengths
    const bool bad = L > stride;       // longer than its slot: neither read nor written, done 0
    const uint32_t Lc = bad ? 0u : L;  // the bytes this slot reads
    const uint32_t nch = (Lc + 15u) >> 4;
    const uint32_t cmax = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_max(nch), 63);
    if (w == 0) t.sum[lane] = 0;  // flushes add
    __syncthreads();
    const buf_t rb = buf_rsrc(arena + b0 * stride, nb * stride);  // the block's slots: its loads and its stores
    if (cmax <= 32) {
        if (cmax <= 8)
            ring_short<8, U>(t, rb, stride, nb, Lc, w, 4u, lane);
        else if (cmax <= 16)
            ring_short<16, U>(t, rb, stride, nb, Lc, w, 4u, lane);
        else
            ring_short<32, U>(t, rb, stride, nb, Lc, w, 4u, lane);
    } else {
        const uint32_t R = (nch + 63u) >> 6;
        const uint32_t incl = wave_incl_scan(R);
        const uint32_t excl = incl - R;
        const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);  // the block's items
        const bool coop = (kflags & kRingAllCoop) || (!(kflags & kRingOwnSlots) && T >= kRingCoopRows * nb);
        if (coop) {  // the four waves on all the block's slots
            ring_rows<UD>(t, rb, stride, Lc, incl, excl, w, T, 4u, lane);
        } else {  // wave w: the items of its quarter of the slots
            const uint32_t q = B / 4u;
            const uint32_t ib = (uint32_t)__builtin_amdgcn_readlane((int)excl, (int)(q * w));
            const uint32_t ie = w < 3 ? (uint32_t)__builtin_amdgcn_readlane((int)excl, (int)(q * w + q)) : T;
            ring_rows<U>(t, rb, stride, Lc, incl, excl, ib, ie, 1u, lane);
        }
    }
    __syncthreads();
    if (w != 0) return;  // wave 0 fills the block's slots
    TxFill fill{0u, 0u, 0u, 0u};
    if (valid && !bad) {
        const uint32_t F = bswap16(fold16(t.sum[lane]));  // slots start 16-byte aligned: even address
        uint32_t hw[24];
#pragma unroll
        for (int k = 0; k < 6; k++) {  // chunks past the frame were never captured: zero
            const u32x4 x = 16u * k < L ? t.hdr[k][lane] : u32x4{0u, 0u, 0u, 0u};
            hw[4 * k] = x.x, hw[4 * k + 1] = x.y, hw[4 * k + 2] = x.z, hw[4 * k + 3] = x.w;
        }
        fill = tx_from_window(arena + (b0 + (uint32_t)lane) * stride, L, F, hw, flags);
    }
    // both values are known: memory gets the big-endian bytes
    const uint32_t at = (uint32_t)lane * stride;
    if (fill.done & kTxIp) store_field16(rb, at + 10u, bswap16(fill.ip_val));
    if (fill.done & kTxL4) store_field16(rb, at + fill.l4_at, bswap16(fill.l4_val));
    refuse(err, bad);
    store_result8(buf_rsrc(done + b0, nb), (uint32_t)lane, fill.done);
}

// pipck_tx_fill_ring: launch_ring_rx's argument rules plus the flags, then one
// k_ring_tx<8, 12> over blocks of 64 slots -- nothing allocated, no ring
// remembered (the RX ring's feedback is not used), so the call can be captured
int launch_ring_tx(void* d_arena, uint64_t stride, const uint16_t* d_lens, uint64_t n, uint32_t flags,
                   uint8_t* d_done, uint32_t* d_err, hipStream_t s) {
    if (flags & ~(uint32_t)PIPCK_TX_UDP_ZERO_AS_ONES) {
        set_error("pipck_tx_fill_ring: unknown flag bits");
        return PIPCK_EINVAL;
    }
    if (n == 0) return PIPCK_OK;
    if (!d_arena || !d_lens || !d_done) {
        set_error("pipck_tx_fill_ring: null pointer");
        return PIPCK_EINVAL;
    }
    if ((uintptr_t)d_arena % 16 || stride % 16 || stride < 1024 || stride > 65536) {
        set_error("pipck_tx_fill_ring: the arena must be 16-byte aligned and the slot stride a multiple of 16 "
                  "bytes from 1 KiB to 64 KiB");
        return PIPCK_EINVAL;
    }
    const uint64_t blocks = (n + kRingB - 1) / kRingB;
    if (blocks > 0x7FFFFFFFull) {
        set_error("pipck_tx_fill_ring: too many slots for one launch");
        return PIPCK_ERANGE;
    }
    const uint32_t mode = tune_now().ring_mode & (kRingOwnSlots | kRingAllCoop);
    PIPCK_LAUNCH((k_ring_tx<8, 12>), dim3((uint32_t)blocks), dim3(256), 0, s, (uint8_t*)d_arena, (uint32_t)stride,
                 d_lens, n, flags, d_done, d_err, mode);
    PIPCK_LAUNCHED("k_ring_tx");
    return PIPCK_OK;
}

}  // namespace pipck

extern "C" {

int pipck_tx_fill_ring(void* d_arena, uint64_t slot_stride, const uint16_t* d_lens, uint64_t n, uint32_t flags,
                       uint8_t* d_done, uint32_t* d_err, void* stream) {
    return pipck::launch_ring_tx(d_arena, slot_stride, d_lens, n, flags, d_done, d_err, pipck::as_stream(stream));
}

}  // extern "C"

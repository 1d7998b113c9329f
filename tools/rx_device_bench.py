#!/usr/bin/env python3
"""Rate of pipck_rx_verify_device: received IP packets already in HBM, byte-packed.

    python tools/rx_device_bench.py [--packets 8388608] [--iters 10] [--warm 40]

Synthetic frames built on the device (engine.gen_rx_frames): cfg4's Zipf L4
lengths (64-9,000 B, the same generator), half TCP/IPv4, a quarter UDP/IPv4, a
quarter TCP/IPv6, every other byte random, checksum fields filled in by the
engine's ragged kernel -- so the verdict histogram is all 7 (PIPCK_RX_VERIFIED)
but for UDP/IPv4 frames whose checksum came out 0 (3, unchecked).  Reports, one JSON line each: pass 1 alone
(k_packedb over the frames, no pseudo-header: pipck_checksum_packed_bytes) and
the whole verifier (k_packedb<RX>: the same stream with each tile's headers
parsed and judged at its end), as frame bytes per second vs the 8 TB/s HBM
peak; algorithmic bytes = frame bytes read + the 2-B sum / 1-B verdict
written per packet.

    python tools/rx_device_bench.py --tx-mixes 64,1500,9000,0

times pipck_tx_fill_device (k_packedb_tx) against pipck_rx_verify_device
(k_packedb_rx) on the same arenas in one process: per mix (an L4 length for every
frame, 0 = the Zipf mix) the legs RX, TX, RX again rotate over the rounds, so the
two RX medians give the run-to-run spread the TX / RX ratio is read against.  The
frames already carry pip's checksums, so the TX leg must leave the arena byte for
byte as it was (checked), whatever it costs to store them again.  One JSON line
per mix, with the library's sha256.

    python tools/rx_device_bench.py --tx-rings

does the same for pipck_tx_fill_ring (k_ring_tx) on the five rings of --rings
(engine.gen_rx_ring: sparse 9,216, dense 1,536, dense 9,216, short 2,048, short
1,024): the yardstick is pipck_rx_verify_ring_n's k_ring on the same ring (tune
ring_adapt=False: k_ring at every fill) in the same process, the legs RX, TX, RX
rotating over six rounds of 20 launches after 40 warm-up launches each; every TX
launch stores every field again and must leave the ring as it was (checked).
One JSON line per ring, with the device's PCI bus id and the library's sha256.

    python tools/rx_device_bench.py --fwd-rings

times pipck_fwd_rewrite_ring (k_fwd_ring; one rule per family with all five ops,
PIPCK_FWD_UDP_ZERO_AS_ONES) against pipck_tx_fill_ring and k_ring on the same
five rings in one process: the legs RX, rewrite, TX, RX rotate over eight rounds
of 20 launches after 40 warm-up launches each.  The rewrite reads header lines
only, so its time follows the slots, not the frame bytes.  Every frame first gets
TTL / hop limit 255 and its checksums filled again, and every leg starts from a
copy of that ring: a rewrite decrements every TTL, and none may expire within a
leg.  After a leg of rewrites pipck_rx_verify_ring_n must give every frame the
verdict it had (checked).  One JSON line per ring.

    python tools/rx_device_bench.py --fwd-device

times pipck_fwd_rewrite_device (k_fwd_device; the same two rules and flag) on
byte-packed arenas (--fwd-mixes: an L4 length for every frame, 0 = the Zipf mix;
with 20- and 40-byte IP headers 64, 1500 and 8900 give frames whose lengths are
all multiples of 4, so every frame starts 4-aligned and takes dword stores, and
1499 gives every start residue: halfword and single-byte stores) against
pipck_rx_verify_device and pipck_tx_fill_device on the same arena and against
pipck_fwd_rewrite_ring on the same frames in ring slots (each frame's first 96
bytes copied into a slot: the ring call reads nothing else of a frame).  The legs
RX, rewrite, TX, ring rewrite, RX rotate over eight rounds of 20 launches after
40 warm-up launches each, every leg from a copy of the same arena and ring, every
frame with TTL / hop limit 255 and DONE under all five ops.  One rewrite of each
layout must give the same bytes and done values, and after a leg of rewrites
pipck_rx_verify_device must give every frame the verdict it had (both checked).
One JSON line per arena, with each leg's rounds and their spread.

    python tools/rx_device_bench.py --fwd-classify

times pipck_fwd_classify_ring / pipck_fwd_classify_device (k_fwd_classify_ring,
k_fwd_classify_device) on the same --rings and --fwd-mixes against the RX verifier
and the rewrite of the same layout, the same rotation: the legs RX, classify
(every frame a hit), classify (the keys removed: every frame a miss at its first
entry), classify (a table as full of keys no frame has: a miss walks to an empty
entry), rewrite, RX over eight rounds of 20 launches after 40 warm-up launches
each.  Every frame first gets the addresses and ports of one of 32,766 bindings
drawn at random (a third each IPv4 TCP, IPv4 UDP, IPv6 TCP), TTL / hop limit 255
and its checksums filled again; the table has 65,536 slots (load 0.5).  Before
anything is timed each table's results are checked on the whole batch (all hits
with the family's rule / all misses with miss_rule) and the arena compared with
what it held.  One JSON line per ring and arena.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def traffic_ratio(tag: str, kernel: str, algo_bytes: int) -> dict:
    """PMC traffic of this kernel on this workload, per launch, from
    profiles/traffic_rx_<tag>.json (tools/pmc_rx.sh writes it with the library's
    sha256): {"traffic": bytes, "traffic_ratio": traffic / algorithmic bytes} when the
    file was measured on this kernel of this build, else {}."""
    import hashlib

    f = ROOT / "profiles" / f"traffic_rx_{tag}.json"
    if not f.exists():
        return {}
    t = json.loads(f.read_text())
    lib = ROOT / "pip_amd" / "lib" / "libpipck.so"
    sha = hashlib.sha256(lib.read_bytes()).hexdigest() if lib.exists() else None
    if t.get("lib_sha256") != sha or t.get("kernel", "").split("(")[0] != kernel.split("(")[0]:
        return {"traffic": None, "traffic_note": "traffic file from another build or kernel"}
    tb = t["hbm_bytes_per_launch"]
    return {"traffic": tb, "traffic_ratio": round(tb / algo_bytes, 4)}


def tx_vs_rx(a):
    """The --tx-mixes legs (see the module docstring)."""
    import hashlib

    import numpy as np
    import torch

    from bench import last_kernel
    from pip_amd import engine
    from size_scan import timed_b2b

    engine.require_gpu()
    from pip_amd import _lib

    sha = hashlib.sha256(_lib.LIBPIPCK.read_bytes()).hexdigest()  # the build this process loaded
    for l4 in [int(x) for x in a.tx_mixes.split(",")]:
        n = a.packets if l4 == 0 else min(a.packets, (8 << 30) // (l4 + 30))  # at most ~8 GiB of frames
        arena, lens, tile_off, _, _, _ = engine.gen_rx_frames(n, 11, l4_len=l4)
        total, nbytes = int(tile_off[-1].item()), arena.numel()
        ok = torch.empty(n, dtype=torch.uint8, device="cuda")
        done = torch.empty(n, dtype=torch.uint8, device="cuda")
        before = arena.clone()

        def rx():
            engine.call("pipck_rx_verify_device", engine._ptr(arena), nbytes, engine._ptr(lens), engine._ptr(tile_off),
                        n, engine._ptr(ok), None, engine.current_stream())

        def tx():
            engine.call("pipck_tx_fill_device", engine._ptr(arena), nbytes, engine._ptr(lens), engine._ptr(tile_off),
                        n, 0, engine._ptr(done), None, engine.current_stream())

        legs = [("rx_a", rx), ("tx", tx), ("rx_b", rx)]
        ms = {k: [] for k, _ in legs}
        kern = {}
        for rnd in range(a.rounds):
            for name, fn in legs[rnd % 3:] + legs[:rnd % 3]:
                for _ in range(a.warm):
                    fn()
                ms[name].append(timed_b2b(fn, a.iters))
                kern[name] = last_kernel().split("(")[0]
        unchanged = bool(torch.equal(arena, before))
        med = {k: statistics.median(v) for k, v in ms.items()}
        rx_mean = (med["rx_a"] + med["rx_b"]) / 2
        hist = lambda t: {int(k): int(c) for k, c in zip(*np.unique(t.cpu().numpy(), return_counts=True))}  # noqa: E731
        print(json.dumps({"what": "tx_fill_device_vs_rx_verify_device", "l4_len": l4 or "zipf", "packets": n,
                          "frame_bytes": total, "rx_kernel": kern["rx_a"], "tx_kernel": kern["tx"],
                          **{k + "_ms": round(v, 4) for k, v in med.items()},
                          **{k + "_rounds_ms": [round(x, 4) for x in v] for k, v in ms.items()},
                          "tx_over_rx": round(med["tx"] / rx_mean, 4),
                          "rx_spread": round(abs(med["rx_a"] - med["rx_b"]) / rx_mean, 4),
                          "tx_GBps": round((total + n) / med["tx"] / 1e6, 1),
                          "tx_frac": round((total + n) / med["tx"] / 1e6 / 8000, 4),
                          "arena_unchanged_by_tx": unchanged, "done": hist(done), "verdicts": hist(ok),
                          "lib_sha256": sha}), flush=True)
        assert unchanged, "pipck_tx_fill_device changed frames that already carried pip's checksums"
        del arena, before, lens, tile_off, ok, done
        torch.cuda.empty_cache()


# the five rings of DESIGN.md section 9 f2: (tag, slot stride, L4 length (0 = Zipf), slots per --packets slot)
BENCH_RINGS = (("ring_sparse_9216", 9216, 0, 1), ("ring_dense_1536", 1536, 1480, 1), ("ring_dense_9216", 9216, 8900, 2),
               ("ring_short_2048", 2048, 200, 1), ("ring_short_1024", 1024, 100, 1))


def tx_rings(a):
    """The --tx-rings legs (see the module docstring)."""
    import hashlib

    import numpy as np
    import torch

    from bench import last_kernel
    from pip_amd import _lib, engine
    from size_scan import timed_b2b

    engine.require_gpu()
    sha = hashlib.sha256(_lib.LIBPIPCK.read_bytes()).hexdigest()  # the build this process loaded
    box = engine.pci_bus_id(torch.cuda.current_device())
    engine.tune(ring_adapt=False)  # RX: k_ring at every fill (k_ring_tx reads no adapt bit)
    try:
        for tag, stride, l4_len, div in [r for r in BENCH_RINGS if r[0] in a.rings.split(",")]:
            m = a.packets // div
            ring, lens, _ = engine.gen_rx_ring(m, 11, stride, l4_len=l4_len)
            fbytes = int((lens.to(torch.int64) & 0xFFFF).sum().item())
            ok = torch.empty(m, dtype=torch.uint8, device="cuda")
            done = torch.empty(m, dtype=torch.uint8, device="cuda")
            before = ring.clone()

            def rx():
                engine.call("pipck_rx_verify_ring_n", engine._ptr(ring), stride, engine._ptr(lens), m, engine._ptr(ok),
                            None, engine.current_stream())

            def tx():
                engine.call("pipck_tx_fill_ring", engine._ptr(ring), stride, engine._ptr(lens), m, 0,
                            engine._ptr(done), None, engine.current_stream())

            legs = [("rx_a", rx), ("tx", tx), ("rx_b", rx)]
            ms = {k: [] for k, _ in legs}
            kern = {}
            for rnd in range(a.rounds):
                for name, fn in legs[rnd % 3:] + legs[:rnd % 3]:
                    for _ in range(a.warm):
                        fn()
                    ms[name].append(timed_b2b(fn, a.iters))
                    kern[name] = last_kernel().split("(")[0]
            unchanged = bool(torch.equal(ring, before))
            med = {k: statistics.median(v) for k, v in ms.items()}
            rx_mean = (med["rx_a"] + med["rx_b"]) / 2
            hist = lambda t: {int(k): int(c) for k, c in zip(*np.unique(t.cpu().numpy(), return_counts=True))}  # noqa: E731
            stores = sum(c * bin(k).count("1") for k, c in hist(done).items())  # one 16-bit store per filled field
            print(json.dumps({"what": "tx_fill_ring_vs_rx_verify_ring", "ring": tag, "slot_stride": stride,
                              "l4_len": l4_len or "zipf", "frames": m, "frame_bytes": fbytes, "slot_bytes": m * stride,
                              "rx_kernel": kern["rx_a"], "tx_kernel": kern["tx"],
                              **{k + "_ms": round(v, 4) for k, v in med.items()},
                              **{k + "_rounds_ms": [round(x, 4) for x in v] for k, v in ms.items()},
                              "tx_over_rx": round(med["tx"] / rx_mean, 4),
                              "rx_spread": round(abs(med["rx_a"] - med["rx_b"]) / rx_mean, 4),
                              "tx_minus_rx_ps_per_frame": round((med["tx"] - rx_mean) * 1e9 / m, 1),
                              "field_stores": stores, "tx_GBps": round((fbytes + m) / med["tx"] / 1e6, 1),
                              "tx_frac": round((fbytes + m) / med["tx"] / 1e6 / 8000, 4),
                              "warm": a.warm, "rounds": a.rounds, "iters": a.iters,
                              "ring_unchanged_by_tx": unchanged, "done": hist(done), "verdicts": hist(ok),
                              "pci_bus_id": box, "lib_sha256": sha}), flush=True)
            assert unchanged, "pipck_tx_fill_ring changed frames that already carried pip's checksums"
            del ring, before, lens, ok, done
            torch.cuda.empty_cache()
    finally:
        engine.tune()


def fwd_rings(a):
    """The --fwd-rings legs (see the module docstring)."""
    import hashlib

    import numpy as np
    import torch

    from bench import last_kernel
    from pip_amd import _lib, engine
    from size_scan import timed_b2b

    engine.require_gpu()
    sha = hashlib.sha256(_lib.LIBPIPCK.read_bytes()).hexdigest()  # the build this process loaded
    box = engine.pci_bus_id(torch.cuda.current_device())
    all_ops = (engine.FWD_SET_SRC | engine.FWD_SET_DST | engine.FWD_SET_SPORT | engine.FWD_SET_DPORT |
               engine.FWD_DEC_TTL)
    rules = engine.make_fwd_rules([
        dict(ops=all_ops, family=4, src=bytes([203, 0, 113, 7]), dst=bytes([198, 51, 100, 9]), sport=40001, dport=53),
        dict(ops=all_ops, family=6, src=bytes.fromhex("20010db885a3000000008a2e03707334"),
             dst=bytes.fromhex("20010db8000000000000ff0000428329"), sport=40001, dport=53)])
    engine.tune(ring_adapt=False)  # RX: k_ring at every fill
    try:
        for tag, stride, l4_len, div in [r for r in BENCH_RINGS if r[0] in a.rings.split(",")]:
            m = a.packets // div
            ring, lens, kind = engine.gen_rx_ring(m, 11, stride, l4_len=l4_len)
            fbytes = int((lens.to(torch.int64) & 0xFFFF).sum().item())
            ok = torch.empty(m, dtype=torch.uint8, device="cuda")
            done = torch.empty(m, dtype=torch.uint8, device="cuda")
            fdone = torch.empty(m, dtype=torch.uint8, device="cuda")
            v6 = kind == 3
            rule_of = v6.to(torch.int32)
            # TTL / hop limit 255 (a leg's launches never reach 1), the checksums filled again
            rows = ring.view(m, stride)
            rows[torch.nonzero(~v6).flatten(), 8] = 255
            rows[torch.nonzero(v6).flatten(), 7] = 255
            engine.tx_fill_ring(ring, stride, lens, m)
            before = ring.clone()
            assert a.warm + a.iters < 250

            def rx():
                engine.call("pipck_rx_verify_ring_n", engine._ptr(ring), stride, engine._ptr(lens), m, engine._ptr(ok),
                            None, engine.current_stream())

            def tx():
                engine.call("pipck_tx_fill_ring", engine._ptr(ring), stride, engine._ptr(lens), m, 0,
                            engine._ptr(done), None, engine.current_stream())

            def fwd():
                engine.call("pipck_fwd_rewrite_ring", engine._ptr(ring), stride, engine._ptr(lens), m,
                            engine._ptr(rules), 2, engine._ptr(rule_of), engine.FWD_UDP_ZERO_AS_ONES,
                            engine._ptr(fdone), None,
                            engine.current_stream())

            rx()
            verdicts_before = ok.clone()
            legs = [("rx_a", rx), ("fwd", fwd), ("tx", tx), ("rx_b", rx)]
            ms = {k: [] for k, _ in legs}
            kern = {}
            for rnd in range(a.rounds):
                for name, fn in legs[rnd % 4:] + legs[:rnd % 4]:
                    ring.copy_(before)  # every leg on the same bytes: a rewrite decrements every TTL
                    for _ in range(a.warm):
                        fn()
                    ms[name].append(timed_b2b(fn, a.iters))
                    kern[name] = last_kernel().split("(")[0]
            # the sums are preserved: after a leg of rewrites every frame has the verdict it had
            ring.copy_(before)
            for _ in range(a.warm + a.iters):
                fwd()
            rx()
            kept = bool(torch.equal(ok, verdicts_before))
            med = {k: statistics.median(v) for k, v in ms.items()}
            rx_mean = (med["rx_a"] + med["rx_b"]) / 2
            hist = lambda t: {int(k): int(c) for k, c in zip(*np.unique(t.cpu().numpy(), return_counts=True))}  # noqa: E731
            n_done = int((fdone == engine.FWD_DONE).sum().item())
            # lines a rewritten slot touches: the window's (read) are the written ones too -- the header
            # fields of these frames lie in the slot's first 128 bytes
            lines = int(((lens.to(torch.int64) & 0xFFFF).clamp(max=96) + 127).div(128, rounding_mode="floor").sum().item())
            print(json.dumps({"what": "fwd_rewrite_ring_vs_tx_fill_ring_vs_rx_verify_ring", "ring": tag,
                              "slot_stride": stride, "l4_len": l4_len or "zipf", "frames": m, "frame_bytes": fbytes,
                              "slot_bytes": m * stride, "rx_kernel": kern["rx_a"], "tx_kernel": kern["tx"],
                              "fwd_kernel": kern["fwd"],
                              **{k + "_ms": round(v, 4) for k, v in med.items()},
                              **{k + "_rounds_ms": [round(x, 4) for x in v] for k, v in ms.items()},
                              "fwd_over_tx": round(med["fwd"] / med["tx"], 4),
                              "fwd_over_rx": round(med["fwd"] / rx_mean, 4),
                              "tx_over_rx": round(med["tx"] / rx_mean, 4),
                              "rx_spread": round(abs(med["rx_a"] - med["rx_b"]) / rx_mean, 4),
                              "fwd_spread": round((max(ms["fwd"]) - min(ms["fwd"])) / med["fwd"], 4),
                              "fwd_ps_per_frame": round(med["fwd"] * 1e9 / m, 1),
                              "fwd_Mframes_per_s": round(m / med["fwd"] / 1e3, 1),
                              "window_lines": lines, "fwd_line_GBps": round(lines * 128 / med["fwd"] / 1e6, 1),
                              "warm": a.warm, "rounds": a.rounds, "iters": a.iters,
                              "verdicts_kept_by_fwd": kept, "fwd_done": hist(fdone), "frames_done": n_done,
                              "tx_done": hist(done), "verdicts": hist(verdicts_before),
                              "pci_bus_id": box, "lib_sha256": sha}), flush=True)
            assert kept, "pipck_fwd_rewrite_ring changed an RX verdict"
            del ring, rows, before, lens, ok, done, fdone, rule_of, verdicts_before
            torch.cuda.empty_cache()
    finally:
        engine.tune()


def fwd_device(a):
    """The --fwd-device legs (see the module docstring)."""
    import hashlib

    import numpy as np
    import torch

    from bench import last_kernel
    from pip_amd import _lib, engine
    from size_scan import timed_b2b

    engine.require_gpu()
    sha = hashlib.sha256(_lib.LIBPIPCK.read_bytes()).hexdigest()  # the build this process loaded
    box = engine.pci_bus_id(torch.cuda.current_device())
    all_ops = (engine.FWD_SET_SRC | engine.FWD_SET_DST | engine.FWD_SET_SPORT | engine.FWD_SET_DPORT |
               engine.FWD_DEC_TTL)
    rules = engine.make_fwd_rules([
        dict(ops=all_ops, family=4, src=bytes([203, 0, 113, 7]), dst=bytes([198, 51, 100, 9]), sport=40001, dport=53),
        dict(ops=all_ops, family=6, src=bytes.fromhex("20010db885a3000000008a2e03707334"),
             dst=bytes.fromhex("20010db8000000000000ff0000428329"), sport=40001, dport=53)])
    flags = engine.FWD_UDP_ZERO_AS_ONES
    for l4 in [int(x) for x in a.fwd_mixes.split(",")]:
        n = a.packets if l4 == 0 else min(a.packets, (8 << 30) // (l4 + 30))  # at most ~8 GiB of frames
        arena, lens, tile_off, kind, start, _ = engine.gen_rx_frames(n, 11, l4_len=l4)
        total, nbytes = int(tile_off[-1].item()), arena.numel()
        v6 = kind == 3
        rule_of = v6.to(torch.int32)
        # TTL / hop limit 255 (a leg's launches never reach 1), the checksums filled again
        arena[start[~v6] + 8] = 255
        arena[start[v6] + 7] = 255
        engine.tx_fill_device(arena, lens, tile_off)
        before = arena.clone()
        flen = lens.to(torch.int64) & 0xFFFF
        # the same frames in ring slots, for pipck_fwd_rewrite_ring: each frame's first 96 bytes -- the
        # call reads nothing else of a frame, so the rest of a slot stays unwritten
        stride = max(1024, (int(flen.max().item()) + 15) // 16 * 16)
        ring = torch.empty(n * stride, dtype=torch.uint8, device="cuda")
        rows = ring.view(n, stride)
        col = torch.arange(96, device="cuda")
        for lo in range(0, n, 1 << 20):
            hi = min(n, lo + (1 << 20))
            idx = (start[lo:hi, None] + col).clamp(max=nbytes - 1)
            rows[lo:hi, :96] = arena[idx]
        ring_before = ring.clone()
        ok = torch.empty(n, dtype=torch.uint8, device="cuda")
        done = torch.empty(n, dtype=torch.uint8, device="cuda")
        fdone = torch.empty(n, dtype=torch.uint8, device="cuda")
        rdone = torch.empty(n, dtype=torch.uint8, device="cuda")
        assert a.warm + a.iters < 250

        def rx():
            engine.call("pipck_rx_verify_device", engine._ptr(arena), nbytes, engine._ptr(lens), engine._ptr(tile_off),
                        n, engine._ptr(ok), None, engine.current_stream())

        def tx():
            engine.call("pipck_tx_fill_device", engine._ptr(arena), nbytes, engine._ptr(lens), engine._ptr(tile_off),
                        n, 0, engine._ptr(done), None, engine.current_stream())

        def fwd():
            engine.call("pipck_fwd_rewrite_device", engine._ptr(arena), nbytes, engine._ptr(lens),
                        engine._ptr(tile_off), n, engine._ptr(rules), 2, engine._ptr(rule_of), flags,
                        engine._ptr(fdone), None, engine.current_stream())

        def fring():
            engine.call("pipck_fwd_rewrite_ring", engine._ptr(ring), stride, engine._ptr(lens), n, engine._ptr(rules),
                        2, engine._ptr(rule_of), flags, engine._ptr(rdone), None, engine.current_stream())

        rx()
        verdicts_before = ok.clone()
        legs = [("rx_a", rx), ("fwd", fwd), ("tx", tx), ("ring", fring), ("rx_b", rx)]
        ms = {k: [] for k, _ in legs}
        kern = {}
        for rnd in range(a.rounds):
            for name, fn in legs[rnd % 5:] + legs[:rnd % 5]:
                arena.copy_(before)  # every leg on the same bytes: a rewrite decrements every TTL
                ring.copy_(ring_before)
                for _ in range(a.warm):
                    fn()
                ms[name].append(timed_b2b(fn, a.iters))
                kern[name] = last_kernel().split("(")[0]
        # one rewrite of each layout from the same bytes gives the same first 96 bytes and done values
        arena.copy_(before)
        ring.copy_(ring_before)
        fwd()
        fring()
        same = bool(torch.equal(fdone, rdone))
        for lo in range(0, n, 1 << 20):
            hi = min(n, lo + (1 << 20))
            idx = (start[lo:hi, None] + col).clamp(max=nbytes - 1)
            same = same and bool(torch.equal(torch.where(col < flen[lo:hi, None], arena[idx], 0),
                                             torch.where(col < flen[lo:hi, None], rows[lo:hi, :96], 0)))
        # the sums are preserved: after a leg of rewrites every frame has the verdict it had
        for _ in range(a.warm + a.iters - 1):
            fwd()
        rx()
        kept = bool(torch.equal(ok, verdicts_before))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        rx_mean = (med["rx_a"] + med["rx_b"]) / 2
        hist = lambda t: {int(k): int(c) for k, c in zip(*np.unique(t.cpu().numpy(), return_counts=True))}  # noqa: E731
        residues = torch.bincount(start % 4, minlength=4).tolist()
        print(json.dumps({"what": "fwd_rewrite_device_vs_rx_verify_device_vs_tx_fill_device_vs_fwd_rewrite_ring",
                          "l4_len": l4 or "zipf", "frames": n, "frame_bytes": total, "ring_stride": stride,
                          "starts_mod_4": residues,
                          "rx_kernel": kern["rx_a"], "tx_kernel": kern["tx"], "fwd_kernel": kern["fwd"],
                          "ring_kernel": kern["ring"],
                          **{k + "_ms": round(v, 4) for k, v in med.items()},
                          **{k + "_rounds_ms": [round(x, 4) for x in v] for k, v in ms.items()},
                          **{k + "_spread": round(v, 4) for k, v in spread.items()},
                          "fwd_over_rx": round(med["fwd"] / rx_mean, 4),
                          "fwd_over_tx": round(med["fwd"] / med["tx"], 4),
                          "fwd_over_ring": round(med["fwd"] / med["ring"], 4),
                          "rx_minus_fwd_ms": round(rx_mean - med["fwd"], 4),
                          "larger_round_spread_ms": round(max(max(ms["fwd"]) - min(ms["fwd"]),
                                                              max(ms["rx_a"] + ms["rx_b"]) - min(ms["rx_a"] + ms["rx_b"])), 4),
                          "fwd_ps_per_frame": round(med["fwd"] * 1e9 / n, 1),
                          "ring_ps_per_frame": round(med["ring"] * 1e9 / n, 1),
                          "warm": a.warm, "rounds": a.rounds, "iters": a.iters,
                          "verdicts_kept_by_fwd": kept, "same_as_ring": same, "fwd_done": hist(fdone),
                          "verdicts": hist(verdicts_before), "pci_bus_id": box, "lib_sha256": sha}), flush=True)
        assert kept, "pipck_fwd_rewrite_device changed an RX verdict"
        assert same, "pipck_fwd_rewrite_device and pipck_fwd_rewrite_ring differ on the same frames"
        del arena, before, ring, rows, ring_before, lens, tile_off, ok, done, fdone, rdone, rule_of, verdicts_before
        torch.cuda.empty_cache()


FWD_BINDINGS = 10922  # per class (IPv4 TCP, IPv4 UDP, IPv6 TCP): 32,766 keys, load 0.49997 of 65,536 slots
FWD_TABLE_SLOTS = 1 << 16


def _binding_key(engine, b, dport=53):
    """Key b of the --fwd-classify table: class b % 3 (IPv4 TCP, IPv4 UDP, IPv6 TCP), the bytes _bind_frames writes."""
    hi, lo = b >> 8, b & 0xFF
    if b % 3 < 2:
        return engine.fwd_key_bytes(4, 17 if b % 3 == 1 else 6, bytes([10, 0, hi, lo]), bytes([198, 51, 100, lo]),
                                    0x8000 | b, dport)
    return engine.fwd_key_bytes(6, 6, bytes.fromhex("20010db8") + bytes(10) + bytes([hi, lo]),
                                bytes.fromhex("20010db8") + bytes(9) + bytes([0xFF, 0, lo]), 0x8000 | b, dport)


def _bind_frames(torch, buf, at, kind, seed):
    """Give every frame (first byte at buf[at[i]]; kind as engine.gen_rx_frames) the addresses and ports of a
    binding drawn at random from the 3 * FWD_BINDINGS of its class, destination port 53, and TTL / hop limit 255."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    v6 = kind == 3
    b = 3 * torch.randint(0, FWD_BINDINGS, (at.numel(),), device="cuda", generator=g) + \
        torch.where(v6, 2, torch.where(kind == 2, 1, 0))
    hi, lo = (b >> 8).to(torch.uint8), (b & 0xFF).to(torch.uint8)

    def put(mask, col, val):
        idx = at[mask] + col
        buf[idx] = val[mask] if torch.is_tensor(val) else torch.full_like(idx, val, dtype=torch.uint8)

    v4 = ~v6
    for col, val in enumerate((10, 0, hi, lo, 198, 51, 100, lo, hi | 0x80, lo, 0, 53), start=12):
        put(v4, col, val)
    put(v4, 8, 255)
    src6 = (0x20, 0x01, 0x0D, 0xB8) + (0,) * 10 + (hi, lo)
    dst6 = (0x20, 0x01, 0x0D, 0xB8) + (0,) * 9 + (0xFF, 0, lo)
    for col, val in enumerate(src6 + dst6 + (hi | 0x80, lo, 0, 53), start=8):
        put(v6, col, val)
    put(v6, 7, 255)


def fwd_classify(a):
    """The --fwd-classify legs (see the module docstring)."""
    import hashlib

    import torch

    from bench import last_kernel
    from pip_amd import _lib, engine
    from size_scan import timed_b2b

    engine.require_gpu()
    sha = hashlib.sha256(_lib.LIBPIPCK.read_bytes()).hexdigest()  # the build this process loaded
    box = engine.pci_bus_id(torch.cuda.current_device())
    all_ops = (engine.FWD_SET_SRC | engine.FWD_SET_DST | engine.FWD_SET_SPORT | engine.FWD_SET_DPORT |
               engine.FWD_DEC_TTL)
    rules = engine.make_fwd_rules([
        dict(ops=all_ops, family=4, src=bytes([203, 0, 113, 7]), dst=bytes([198, 51, 100, 9]), sport=40001, dport=53),
        dict(ops=all_ops, family=6, src=bytes.fromhex("20010db885a3000000008a2e03707334"),
             dst=bytes.fromhex("20010db8000000000000ff0000428329"), sport=40001, dport=53)])
    flags = engine.FWD_UDP_ZERO_AS_ONES
    n_keys = 3 * FWD_BINDINGS
    rule_of_key = [int(b % 3 == 2) for b in range(n_keys)]  # rule 0: IPv4, rule 1: IPv6
    tables = {"hit": engine.make_fwd_table([_binding_key(engine, b) for b in range(n_keys)], rule_of_key, FWD_TABLE_SLOTS),
              # the keys removed: every search ends at its first entry
              "miss": engine.make_fwd_table([], [], FWD_TABLE_SLOTS),
              # as full as the first, of keys no frame has (destination port 54): a miss walks to an empty entry
              "miss_full": engine.make_fwd_table([_binding_key(engine, b, 54) for b in range(n_keys)], rule_of_key,
                                                 FWD_TABLE_SLOTS)}
    miss_rule = 0x7FFFFFFF
    configs = [("ring", r) for r in BENCH_RINGS if r[0] in a.rings.split(",")] + \
              [("packed", int(x)) for x in a.fwd_mixes.split(",") if x]
    engine.tune(ring_adapt=False)  # RX on rings: k_ring at every fill
    try:
        for layout, cfg in configs:
            if layout == "ring":
                tag, stride, l4, div = cfg
                n = a.packets // div
                arena, lens, kind = engine.gen_rx_ring(n, 11, stride, l4_len=l4)
                at = torch.arange(n, device="cuda") * stride
                _bind_frames(torch, arena, at, kind, 12)
                engine.tx_fill_ring(arena, stride, lens, n)
                head = (engine._ptr(arena), stride, engine._ptr(lens), n)
                names = ("pipck_rx_verify_ring_n", "pipck_fwd_classify_ring", "pipck_fwd_rewrite_ring")
            else:
                l4 = cfg
                tag = f"packed_{l4 or 'zipf'}"
                n = a.packets if l4 == 0 else min(a.packets, (8 << 30) // (l4 + 30))  # at most ~8 GiB of frames
                arena, lens, tile_off, kind, at, _ = engine.gen_rx_frames(n, 11, l4_len=l4)
                _bind_frames(torch, arena, at, kind, 12)
                engine.tx_fill_device(arena, lens, tile_off)
                head = (engine._ptr(arena), arena.numel(), engine._ptr(lens), engine._ptr(tile_off), n)
                names = ("pipck_rx_verify_device", "pipck_fwd_classify_device", "pipck_fwd_rewrite_device")
            fbytes = int((lens.to(torch.int64) & 0xFFFF).sum().item())
            before = arena.clone()
            want_rule = (kind == 3).to(torch.int32)
            ok = torch.empty(n, dtype=torch.uint8, device="cuda")
            fdone = torch.empty(n, dtype=torch.uint8, device="cuda")
            rule_of = torch.empty(n, dtype=torch.int32, device="cuda")
            cls = torch.empty(n, dtype=torch.uint8, device="cuda")
            assert a.warm + a.iters < 250
            stream = engine.current_stream()

            def rx():
                engine.call(names[0], *head, engine._ptr(ok), None, stream)

            def classify(which):
                def fn():
                    engine.call(names[1], *head, engine._ptr(tables[which]), FWD_TABLE_SLOTS, miss_rule,
                                engine.FWD_NO_RULE, engine._ptr(ok), 3, engine._ptr(rule_of), engine._ptr(cls), None,
                                stream)
                return fn

            def fwd():
                engine.call(names[2], *head, engine._ptr(rules), 2, engine._ptr(want_rule), flags, engine._ptr(fdone),
                            None, stream)

            rx()
            gated = int(((ok & 3) != 3).sum().item())
            # what each table gives, before anything is timed: every frame a hit with its family's rule / a miss
            checks = {}
            for which in tables:
                classify(which)()
                want_cls = engine.FWD_CLASS_HIT if which == "hit" else engine.FWD_CLASS_MISS
                checks[which] = bool((cls == want_cls).all().item()) and bool(
                    torch.equal(rule_of, want_rule) if which == "hit" else (rule_of == miss_rule).all().item())
            assert gated == 0 and all(checks.values()), (tag, gated, checks)
            assert torch.equal(arena, before), "a classify call wrote the arena"
            legs = [("rx_a", rx), ("cls_hit", classify("hit")), ("cls_miss", classify("miss")),
                    ("cls_miss_full", classify("miss_full")), ("fwd", fwd), ("rx_b", rx)]
            ms = {k: [] for k, _ in legs}
            kern = {}
            for rnd in range(a.rounds):
                k = rnd % len(legs)
                for name, fn in legs[k:] + legs[:k]:
                    arena.copy_(before)  # every leg on the same bytes: a rewrite decrements every TTL
                    for _ in range(a.warm):
                        fn()
                    ms[name].append(timed_b2b(fn, a.iters))
                    kern[name] = last_kernel().split("(")[0]
            med = {k: statistics.median(v) for k, v in ms.items()}
            rx_all = ms["rx_a"] + ms["rx_b"]
            rx_mean = (med["rx_a"] + med["rx_b"]) / 2
            larger = max(max(ms["cls_hit"]) - min(ms["cls_hit"]), max(rx_all) - min(rx_all))
            print(json.dumps({"what": "fwd_classify_vs_rx_verify_vs_fwd_rewrite", "layout": layout, "config": tag,
                              "l4_len": l4 or "zipf", "frames": n, "frame_bytes": fbytes,
                              "table_slots": FWD_TABLE_SLOTS, "table_keys": n_keys,
                              "rx_kernel": kern["rx_a"], "cls_kernel": kern["cls_hit"], "fwd_kernel": kern["fwd"],
                              **{k + "_ms": round(v, 4) for k, v in med.items()},
                              **{k + "_rounds_ms": [round(x, 4) for x in v] for k, v in ms.items()},
                              "cls_over_rx": round(med["cls_hit"] / rx_mean, 4),
                              "cls_over_fwd": round(med["cls_hit"] / med["fwd"], 4),
                              "rx_minus_cls_ms": round(rx_mean - med["cls_hit"], 4),
                              "larger_round_spread_ms": round(larger, 4),
                              "cls_below_rx_by_more_than_the_spread": bool(rx_mean - med["cls_hit"] > larger),
                              "cls_hit_ps_per_frame": round(med["cls_hit"] * 1e9 / n, 1),
                              "cls_miss_ps_per_frame": round(med["cls_miss"] * 1e9 / n, 1),
                              "cls_miss_full_ps_per_frame": round(med["cls_miss_full"] * 1e9 / n, 1),
                              "fwd_ps_per_frame": round(med["fwd"] * 1e9 / n, 1),
                              "hit_minus_miss_ps_per_frame": round((med["cls_hit"] - med["cls_miss"]) * 1e9 / n, 1),
                              "warm": a.warm, "rounds": a.rounds, "iters": a.iters, "checked": checks,
                              "pci_bus_id": box, "lib_sha256": sha}), flush=True)
            del arena, before, lens, kind, at, ok, fdone, rule_of, cls, want_rule
            torch.cuda.empty_cache()
    finally:
        engine.tune()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=8 << 20)
    ap.add_argument("--iters", type=int, default=None, help="timed launches per round (10; --tx-rings, --fwd-rings: 20)")
    ap.add_argument("--warm", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=None, help="rounds per arm (3; --tx-rings: 6; --fwd-rings: 8)")
    ap.add_argument("--rings", default="ring_sparse_9216,ring_dense_1536,ring_dense_9216,ring_short_2048,ring_short_1024")
    ap.add_argument("--tune", default="{}", help="engine.tune kwargs for the packed arms and the default (groups) ring arm, JSON")
    ap.add_argument("--skip-packed", action="store_true", help="rings only")
    ap.add_argument("--arms", default="groups,kring,rows,slots",
                    help="ring schedules to time; groups:NAME = the default with --tunes[NAME]")
    ap.add_argument("--tunes", default="{}", help='JSON {"NAME": engine.tune kwargs} for groups:NAME arms')
    ap.add_argument("--tx-mixes", default="",
                    help="L4 lengths (0 = Zipf) for the TX-against-RX legs; nothing else runs")
    ap.add_argument("--tx-rings", action="store_true",
                    help="pipck_tx_fill_ring against k_ring on the --rings; nothing else runs")
    ap.add_argument("--fwd-rings", action="store_true",
                    help="pipck_fwd_rewrite_ring against pipck_tx_fill_ring and k_ring on the --rings; nothing else runs")
    ap.add_argument("--fwd-device", action="store_true",
                    help="pipck_fwd_rewrite_device against pipck_rx_verify_device, pipck_tx_fill_device and "
                         "pipck_fwd_rewrite_ring on the --fwd-mixes; nothing else runs")
    ap.add_argument("--fwd-mixes", default="64,1500,8900,0,1499",
                    help="L4 lengths (0 = Zipf) of the --fwd-device arenas")
    ap.add_argument("--fwd-classify", action="store_true",
                    help="pipck_fwd_classify_ring / _device against the RX verifier and the rewrite on the --rings "
                         "and --fwd-mixes; nothing else runs")
    a = ap.parse_args()
    if a.fwd_classify:
        a.iters, a.rounds = a.iters or 20, a.rounds or 8
        return fwd_classify(a)
    if a.fwd_device:
        a.iters, a.rounds = a.iters or 20, a.rounds or 8
        return fwd_device(a)
    if a.fwd_rings:
        a.iters, a.rounds = a.iters or 20, a.rounds or 8
        return fwd_rings(a)
    if a.tx_rings:
        a.iters, a.rounds = a.iters or 20, a.rounds or 6
        return tx_rings(a)
    a.iters, a.rounds = a.iters or 10, a.rounds or 3
    if a.tx_mixes:
        return tx_vs_rx(a)
    tune_default = json.loads(a.tune)
    tunes = json.loads(a.tunes)
    import torch

    from bench import last_kernel
    from pip_amd import engine
    from size_scan import timed_b2b

    engine.require_gpu()
    n = a.packets
    if a.skip_packed:
        arena = lens = tile_off = None
        total = 0
    else:
        arena, lens, tile_off, _, _, _ = engine.gen_rx_frames(n, 11)
        total = int(tile_off[-1].item())
    sums = torch.empty(n, dtype=torch.int16, device="cuda")
    ok = torch.empty(n, dtype=torch.uint8, device="cuda")
    nbytes = arena.numel() if arena is not None else 0

    def pass1():
        engine.call("pipck_checksum_packed_bytes_n", engine._ptr(arena), nbytes, engine._ptr(lens),
                    engine._ptr(tile_off), n, None, 0, None, 0, engine._ptr(sums), None, engine.current_stream())

    def full():
        engine.call("pipck_rx_verify_device", engine._ptr(arena), nbytes, engine._ptr(lens), engine._ptr(tile_off),
                    n, engine._ptr(ok), None, engine.current_stream())

    res = {"pass1": [], "rx_verify_device": []}
    kern = {}
    engine.tune(**tune_default)
    for rnd in range(0 if a.skip_packed else a.rounds):
        for name, fn in (("pass1", pass1), ("rx_verify_device", full)) if rnd % 2 == 0 else \
                (("rx_verify_device", full), ("pass1", pass1)):
            for _ in range(a.warm):
                fn()
            res[name].append(timed_b2b(fn, a.iters))
            kern[name] = last_kernel().split("(")[0]
    engine.tune()
    # rings: frames in fixed-size slots (pipck_rx_verify_ring), sparse (the same
    # Zipf frames in 9,216-B slots), dense (1,480-B L4 in 1,536-B slots, 8,900-B
    # L4 in 9,216-B slots) and short frames in small slots (200-B L4 in 2 KiB,
    # 100-B L4 in 1 KiB)
    rings = (("ring_sparse_9216", 9216, 0, n), ("ring_dense_1536", 1536, 1480, n), ("ring_dense_9216", 9216, 8900, n // 2),
             ("ring_short_2048", 2048, 200, n), ("ring_short_1024", 1024, 100, n),
             # probes (not in the default set): every slot filled to the byte (IPv4 frames of 9,216 B;
             # IPv6 ones 20 B longer would not fit, so the L4 length leaves room for both)
             ("ring_full_9216", 9216, 9216 - 40, n // 2), ("ring_full_1536", 1536, 1536 - 40, n))
    for tag, stride, l4_len, m in [r for r in rings if r[0] in a.rings.split(",")]:  # --rings none: packed only
        del arena
        torch.cuda.empty_cache()
        ring, rlens, _ = engine.gen_rx_ring(m, 11, stride, l4_len=l4_len)
        rok = torch.empty(m, dtype=torch.uint8, device="cuda")
        fbytes = int((rlens.to(torch.int64) & 0xFFFF).sum().item())

        def rfn():
            engine.call("pipck_rx_verify_ring", engine._ptr(ring), stride, engine._ptr(rlens), m, engine._ptr(rok),
                        engine.current_stream())

        # the three schedules, rounds interleaved, verdicts equal: the default slot
        # groups (k_ring), the row stream (k_ring_rx, flag bit 28) and slot by slot
        # (k_ring_slots, the wave-per-packet arm)
        ts = {k: [] for k in a.arms.split(",")}
        got = {}
        for _ in range(a.rounds):
            for arm in ts:
                if arm == "slots":
                    engine.tune(lanes_per_packet=256)
                elif arm == "rows":
                    engine.tune(alt_flat_schedule=True)
                elif arm == "kring":  # k_ring at every fill (no feedback)
                    engine.tune(**{**tune_default, "ring_adapt": False})
                elif arm.startswith("groups:"):
                    engine.tune(**tunes[arm.split(":", 1)[1]])
                else:
                    engine.tune(**tune_default)
                for _ in range(a.warm):
                    rfn()
                ts[arm].append(timed_b2b(rfn, a.iters))
                got[arm] = (last_kernel().split("(")[0], rok.clone())
        engine.tune()
        arms = list(got)
        assert all(torch.equal(got[arms[0]][1], got[k][1]) for k in arms)
        for arm, tl in ts.items():
            mr = statistics.median(tl)
            h = {int(k): int(c) for k, c in zip(*__import__("numpy").unique(got[arm][1].cpu().numpy(), return_counts=True))}
            print(json.dumps({"what": tag, "schedule": arm, "packets": m, "frame_bytes": fbytes,
                              "slot_bytes": m * stride, "last_kernel": got[arm][0], "ms": round(mr, 4),
                              "rounds_ms": [round(x, 4) for x in tl], "GBps": round((fbytes + m) / mr / 1e6, 1),
                              "frac": round((fbytes + m) / mr / 1e6 / 8000, 4), "verdicts": h,
                              **traffic_ratio(tag, got[arm][0], fbytes + m),
                              "verdicts_equal_across_schedules": True}), flush=True)
        del ring
        arena = torch.empty(1, device="cuda")
    if a.skip_packed:
        return
    v = ok.cpu().numpy()
    hist = {int(k): int(c) for k, c in zip(*__import__("numpy").unique(v, return_counts=True))}
    for name, ms in res.items():
        m = statistics.median(ms)
        algo = total + (n if name == "rx_verify_device" else 2 * n)
        print(json.dumps({"what": name, "packets": n, "frame_bytes": total, "last_kernel": kern[name], "ms": round(m, 4),
                          "rounds_ms": [round(x, 4) for x in ms], "GBps": round(algo / m / 1e6, 1),
                          "frac": round(algo / m / 1e6 / 8000, 4), **traffic_ratio(name, kern[name], algo),
                          **({"verdicts": hist} if name == "rx_verify_device" else {})}), flush=True)


if __name__ == "__main__":
    main()

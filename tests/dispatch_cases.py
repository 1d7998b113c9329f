"""The case table of tests/test_gpu_dispatch.py: which kernel instantiation every
entry point launches, with one tuning knob moved from its default at a time.

A GROUP is one entry point on one batch shape; a KNOB is one setting of the
internal tuning words (pipck_testing.h).  run_group makes one launch per knob and
returns {knob id: [return code, kernel name]}, the name as pipck_last_launch
gives it, cut at the closing '>' of its template arguments (None when the call
launched nothing).  run_group looks at no result: every output goes to a scratch
buffer, and the measurement bits (21-23, the in-place probe) compute none.
tests/test_gpu_dispatch_results.py makes the same launches, knob for knob
(apply_knob / reset_knobs), on batches with real contents and holds every result
to a reference; tests/dispatch_results.py has those contents and references.

Run as a program, this writes the table a build produces as JSON:

    PIPCK_LIB=/path/to/libpipck.so python -m tests.dispatch_cases out.json --parent <commit>

tests/golden/dispatch.json was written that way by a build of the commit it
names, in a process of its own.
"""
from __future__ import annotations

import ctypes as C
import json
import sys

LOADS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 24, 25, 28, 32, 33, 48, 72, 74)
FLAG_BITS = tuple(range(0, 8)) + tuple(range(16, 24)) + tuple(range(28, 32))
ROWS = (2, 64, 96)  # rows_per_task values the parity and verify tests already pass
ALT = 1 << 28
RING_NO_FEEDBACK = 1 << 2  # with the feedback the ring verifier's choice depends on the launch history, by design

# (stride, len, n, byte offset of the arena)
FIXED_SHAPES = [(20, 20, 4099, 0), (24, 24, 4099, 0), (24, 20, 4099, 0), (40, 40, 4099, 0), (64, 64, 4099, 0),
                (512, 512, 4099, 0), (1024, 1024, 4099, 0), (1488, 1488, 4099, 0), (1488, 1488, 4099, 8),
                (1500, 1500, 4099, 0), (2048, 2048, 4099, 0), (4096, 4096, 4099, 0), (9008, 9000, 4099, 0),
                (65536, 65535, 67, 0), (65552, 9000, 67, 0)]
HDR_THRESHOLD = (20, 20, 8 << 20, 0)  # default tune only: crosses k_hdr's batch-size threshold (160 MB)
FIXED_MODES = ("checksum", "checksum_pseudo", "verify", "verify_pseudo")
OTHER_GROUPS = ("ragged_checksum", "ragged_verify", "packed_checksum", "packed_verify", "packed_bytes_checksum",
                "packed_bytes_verify", "rx_verify_device", "chains", "tx_fill")
RING_STRIDES = (1024, 2048, 4096, 9216)
N = 4099


def knob(lanes=0, loads=0, blocks=0, flags=0, ring=0, probes=0, xw=False):
    return dict(lanes=lanes, loads=loads, blocks=blocks, flags=flags, ring=ring, probes=probes, xw=xw)


def general_knobs() -> dict[str, dict]:
    k = {"default": knob()}
    for v in (1, 2, 4, 8, 16, 32, 64, 256):
        k[f"lanes={v}"] = knob(lanes=v)
    for v in LOADS:
        k[f"loads={v}"] = knob(loads=v)
        k[f"bit28,loads={v}"] = knob(loads=v, flags=ALT)
    for v in (1, 8, 16, 32):
        k[f"blocks={v}"] = knob(blocks=v)
    for b in FLAG_BITS:
        k[f"bit{b}"] = knob(flags=1 << b)
    for v in (1, 2, 3, 4):
        k[f"small_k_log={v}"] = knob(flags=v << 24)
    for v in ROWS:
        k[f"rows={v}"] = knob(flags=v << 8)
    k["xcd_weights"] = knob(xw=True)
    k["xcd_weights,bit28"] = knob(xw=True, flags=ALT)  # (k_flat is the other schedule at most strides)
    k["probes=1"] = knob(probes=1)
    k["probes=1,loads=32"] = knob(probes=1, loads=32)  # (k_hdr at any batch size)
    return k


def ring_knobs() -> dict[str, dict]:
    k = {name: dict(v, ring=RING_NO_FEEDBACK) for name, v in general_knobs().items()}
    for name, mode in (("ring_own_slots", 1), ("ring_all_coop", 2)):
        k[name] = knob(ring=RING_NO_FEEDBACK | mode)
        for v in (8, 12, 16, 24, 17, 25):
            k[f"{name},loads={v}"] = knob(ring=RING_NO_FEEDBACK | mode, loads=v)
        for v in (8, 16, 32):
            k[f"{name},blocks={v}"] = knob(ring=RING_NO_FEEDBACK | mode, blocks=v)
    return k


def fixed_id(shape, mode) -> str:
    stride, length, n, off = shape
    return f"fixed_{mode}[{stride},{length},n={n}" + (f",+{off}]" if off else "]")


def groups() -> list[str]:
    g = [fixed_id(s, m) for s in FIXED_SHAPES for m in FIXED_MODES]
    g += [fixed_id(HDR_THRESHOLD, m) for m in FIXED_MODES]
    g += list(OTHER_GROUPS)
    g += [f"rx_verify_ring[{s}]" for s in RING_STRIDES]
    return g


def knob_set(group: str) -> str:
    if group.startswith("rx_verify_ring"):
        return "ring"
    return "default_only" if f"n={HDR_THRESHOLD[2]}" in group else "general"


KNOB_SETS = {"general": general_knobs(), "ring": ring_knobs(), "default_only": {"default": knob()}}


def knobs_of(group: str) -> dict[str, dict]:
    return KNOB_SETS[knob_set(group)]


def encode(results: dict[str, dict[str, list]], built_from) -> dict:
    """The golden file: per group one kernel index per knob, in the order of the group's knob set (-1: the call
    launched nothing; its return code is then under "failed")."""
    names = sorted({name for r in results.values() for _, name in r.values() if name is not None})
    cases = {g: [-1 if r[k][1] is None else names.index(r[k][1]) for k in knobs_of(g)] for g, r in results.items()}
    failed = {g: {k: rc for k, (rc, _) in r.items() if rc} for g, r in results.items()}
    return {"built_from": built_from, "names": names, "knobs": {s: list(k) for s, k in KNOB_SETS.items()},
            "cases": cases, "failed": {g: f for g, f in failed.items() if f}}


def decode(golden: dict, group: str) -> dict[str, list]:
    """{knob id: [return code, kernel name]} of a group, as run_group returns it."""
    knobs = golden["knobs"][knob_set(group)]
    failed = golden["failed"].get(group, {})
    return {k: [failed.get(k, 0), None if i < 0 else golden["names"][i]]
            for k, i in zip(knobs, golden["cases"][group], strict=True)}


class Batches:
    """The device batches the groups launch on, each made on first use."""

    def __init__(self):
        import torch

        from pip_amd import engine
        from pip_amd.workloads import CFG2, CFG4, N_FLOWS

        self.torch, self.engine, self.w4, self.n_flows = torch, engine, CFG4, N_FLOWS
        engine.require_gpu()
        self.pseudo = engine.gen_flows(4, N_FLOWS, CFG2.seed, CFG2.proto)[1]
        self.cache: dict = {}
        big = max(s * n + off for s, _, n, off in FIXED_SHAPES + [HDR_THRESHOLD])
        self.arena = torch.zeros(big + 4096, dtype=torch.uint8, device="cuda")  # every fixed shape is a slice of it
        self.out = torch.zeros(HDR_THRESHOLD[2], dtype=torch.int16, device="cuda")
        self.ok = torch.zeros(HDR_THRESHOLD[2], dtype=torch.uint8, device="cuda")
        self.err = torch.zeros(1, dtype=torch.int32, device="cuda")

    def get(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def launcher(self, group: str):
        """A zero-argument function making the group's one launch."""
        e, w, out, ok, err = self.engine, self.w4, self.out, self.ok, self.err
        if group.startswith("fixed_"):
            mode = group[len("fixed_"):group.index("[")]
            shape = next(s for s in FIXED_SHAPES + [HDR_THRESHOLD] if fixed_id(s, mode) == group)
            stride, length, n, off = shape
            arena = self.arena[off:off + stride * n]
            pseudo = self.pseudo if mode.endswith("_pseudo") else None
            nf = self.n_flows if pseudo is not None else None
            if mode.startswith("verify"):
                return lambda: e.verify_fixed(arena, stride, length, n, pseudo, nf, ok=ok, err=err)
            return lambda: e.checksum_fixed(arena, stride, length, n, pseudo, nf, out=out, err=err)
        if group.startswith("ragged_"):
            arena, desc, _ = self.get("ragged", lambda: e.gen_ragged(N, 0, w.seed, w.hdr, self.n_flows))
            if group.endswith("verify"):
                return lambda: e.verify_ragged(arena, desc, self.pseudo, ok=ok, err=err)
            return lambda: e.checksum_ragged(arena, desc, self.pseudo, out=out, err=err)
        if group.startswith("packed_bytes_"):
            arena, lens, tile_off, _ = self.get("packed_bytes", lambda: e.gen_packed_bytes(N, 0, w.seed, w.hdr))
            f = e.verify_packed_bytes if group.endswith("verify") else e.checksum_packed_bytes
            res = dict(ok=ok) if group.endswith("verify") else dict(out=out)
            return lambda: f(arena, lens, tile_off, N, self.pseudo, self.n_flows, err=err, **res)
        if group.startswith("packed_"):
            arena, lens, tile_chunk, _ = self.get("packed", lambda: e.gen_packed(N, 0, w.seed, w.hdr))
            f = e.verify_packed if group.endswith("verify") else e.checksum_packed
            res = dict(ok=ok) if group.endswith("verify") else dict(out=out)
            return lambda: f(arena, lens, tile_chunk, N, self.pseudo, self.n_flows, err=err, **res)
        if group == "rx_verify_device":
            arena, lens, tile_off = self.get("rx", lambda: e.gen_rx_frames(N, 77))[:3]
            return lambda: e.rx_verify_device(arena, lens, tile_off, N, ok=ok, err=err)
        if group == "tx_fill":
            arena, lens, tile_off = self.get("tx", lambda: e.gen_rx_frames(N, 78, checksummed=False))[:3]
            return lambda: e.tx_fill_device(arena, lens, tile_off, N, done=ok, err=err)
        if group == "chains":
            arena, desc, _ = self.get("ragged", lambda: e.gen_ragged(N, 0, w.seed, w.hdr, self.n_flows))
            t = self.torch
            begin = self.get("chain_begin", lambda: t.tensor(list(range(0, N, 3)) + [N], dtype=t.int64, device="cuda"))
            flow = self.get("chain_flow", lambda: t.zeros(begin.numel() - 1, dtype=t.int32, device="cuda"))
            return lambda: e.checksum_chains(arena, desc, begin, flow, self.pseudo, out=out, err=err)
        if group.startswith("rx_verify_ring"):
            stride = int(group[group.index("[") + 1:-1])
            ring, lens, _ = self.get(group, lambda: e.gen_rx_ring(N, 31, stride, l4_len=stride - 300))
            return lambda: e.rx_verify_ring(ring, stride, lens, N, ok=ok, err=err)
        raise KeyError(group)


def last_kernel() -> str:
    from pip_amd import _lib

    buf = C.create_string_buffer(4096)
    _lib.check("pipck_last_launch", _lib.load().pipck_last_launch(buf, len(buf)))
    return buf.value.decode().split("(")[0]


def apply_knob(k: dict, xw: bool) -> bool:
    """Set the tuning words of knob k (pipck_tune, pipck_tune_probes, pipck_tune_ring, the XCD weights).
    xw: whether the XCD weights are on now; returns whether they are on afterwards."""
    from pip_amd import _lib, engine

    lib = _lib.load()
    lib.pipck_tune(k["lanes"], k["loads"], k["blocks"], k["flags"])
    lib.pipck_tune_probes(k["probes"])
    lib.pipck_tune_ring(k["ring"])
    if k["xw"] != xw:  # (a synchronous copy to the device: only when it changes)
        xw = k["xw"]
        engine.tune_xcd_weights([7] * 8 if xw else None, 7 if xw else 0)
    return xw


def reset_knobs() -> None:
    """Every tuning word back to its default."""
    from pip_amd import engine

    engine.tune_xcd_weights(None, 0)
    engine.tune()


def run_group(batches: Batches, group: str) -> dict[str, list]:
    from pip_amd import _lib

    launch = batches.launcher(group)
    got = {}
    xw = False
    try:
        for name, k in knobs_of(group).items():
            xw = apply_knob(k, xw)
            try:
                launch()
                got[name] = [0, last_kernel()]
            except _lib.PipckError as ex:
                got[name] = [ex.rc, None]
        batches.torch.cuda.synchronize()
    finally:
        reset_knobs()
    return got


def main(argv) -> int:
    import subprocess

    out = argv[1] if len(argv) > 1 else "dispatch.json"
    parent = argv[argv.index("--parent") + 1] if "--parent" in argv else None
    if parent is None:
        parent = subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    batches = Batches()
    golden = encode({g: run_group(batches, g) for g in groups()}, parent)
    with open(out, "w") as f:  # one group per line
        head = {k: v for k, v in golden.items() if k != "cases"}
        rows = ",\n".join(f"{json.dumps(g)}:{json.dumps(c, separators=(',', ':'))}" for g, c in golden["cases"].items())
        f.write(json.dumps(head, separators=(",", ":"))[:-1] + ',\n"cases":{\n' + rows + "\n}}\n")
    print(f"{sum(len(c) for c in golden['cases'].values())} launches in {len(golden['cases'])} groups, "
          f"{len(golden['names'])} kernels -> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

"""CPU: the ABI of pipck_fwd_rewrite_device (include/pipck.h) -- the header's
declaration, the version, the ctypes signature, the exported symbol and the
argument rules that need no device -- and the SHORT SET of the GPU tests
(tests/test_gpu_fwd_device.py) with its census by tests/fwd_reference.py alone:
frames of 20 to 51 bytes back to back, the smallest input at which two or three
frames' fields share one 16-byte chunk and a neighbour's bytes the dword of a
stored field."""
import ctypes as C
import functools
import random
import re
from pathlib import Path

import numpy as np

from tests import fwd_reference as F
from tests import rx_reference as R
from tests.test_fwd_reference import assign, reference_rewrite

ROOT = Path(__file__).resolve().parents[1]
NAME = "pipck_fwd_rewrite_device"


@functools.lru_cache(maxsize=None)
def short_set():
    """Six repetitions over family 4 and 6 of the shortest TCP (L4 length 20), UDP (8) and ICMP /
    ICMPv6 (8) frames, checksums filled, each followed by 0, 1, 2 and 3 bytes of link padding;
    after every fifth frame a random frame of 0 to 15 bytes, after every seventh a bare 20-byte
    IPv4 header with protocol 253 and 0 to 3 bytes of padding."""
    rng = random.Random(1624)
    frames, made = [], 0
    for _ in range(6):
        for fam in (4, 6):
            for proto, l4len in ((R.TCP, 20), (R.UDP, 8), (R.ICMP if fam == 4 else R.ICMP6, 8)):
                for pad in range(4):
                    frames.append(R.build(rng, fam, proto, l4len, fill=True) + rng.randbytes(pad))
                    made += 1
                    if made % 5 == 0:
                        frames.append(rng.randbytes(rng.randrange(16)))
                    if made % 7 == 0:
                        frames.append(R.build(rng, 4, 253, 0) + rng.randbytes(rng.randrange(4)))
    return tuple(frames)


def short_starts(frames, lead=0):
    return lead + np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)[:-1]


def test_short_set_census():
    frames = short_set()
    assert 190 <= len(frames) <= 210 and 6000 <= sum(map(len, frames)) <= 8000
    assert sum(20 <= len(f) <= 51 for f in frames) >= 100 and max(map(len, frames)) <= 63
    done = reference_rewrite(frames, assign(frames), 0)[1]
    counts = {v: int((done == v).sum()) for v in (F.DONE, F.UNHANDLED, 0, F.EXPIRED)}
    print("short set census", len(frames), sum(map(len, frames)), counts)
    assert counts[F.DONE] >= 100, counts
    assert counts[F.UNHANDLED] >= 10 and counts[0] >= 20, counts
    starts = short_starts(frames)
    by_residue = np.bincount(starts[done == F.DONE] % 16, minlength=16)
    print("DONE frames per start residue mod 16", by_residue.tolist())
    assert by_residue.min() >= 1, by_residue
    # what makes the set the short set: a DONE frame shares its first or last dword with a neighbour
    ends = starts + np.array([len(f) for f in frames])
    assert sum(1 for i in np.nonzero(done == F.DONE)[0] if starts[i] % 4 or ends[i] % 4) >= 50


def test_abi_declares_and_exports_fwd_rewrite_device():
    from pip_amd import _lib

    raw = (ROOT / "include" / "pipck.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, text)
    assert m, "include/pipck.h does not declare " + NAME
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 12
    assert [p.split()[-1].lstrip("*") for p in params] == ["d_arena", "arena_bytes", "d_lens", "d_tile_off", "n_packets",
                                                           "d_rules", "n_rules", "d_rule_of", "flags", "d_done",
                                                           "d_err", "stream"]
    assert int(re.search(r"#define PIPCK_VERSION_MINOR (\d+)", text).group(1)) >= 7
    assert "1.7: " + NAME in re.sub(r"\s+", " ", raw)
    restype, argtypes = _lib.SIGNATURES[NAME]
    p, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    assert restype is C.c_int and list(argtypes) == [p, u64, p, p, u64, p, u32, p, u32, p, p, p]
    lib = _lib.load()
    assert hasattr(lib, NAME)
    assert lib.pipck_version() >> 16 == 1 and lib.pipck_version() & 0xFFFF >= 7
    fn = getattr(lib, NAME)
    # n_packets == 0: PIPCK_OK before any pointer check, but the flag check comes first
    assert fn(None, 0, None, None, 0, None, 0, None, 0, None, None, None) == _lib.PIPCK_OK
    assert fn(None, 0, None, None, 0, None, 0, None, 1, None, None, None) == _lib.PIPCK_OK
    assert fn(None, 0, None, None, 0, None, 0, None, 2, None, None, None) == _lib.PIPCK_EINVAL
    assert NAME.encode() in lib.pipck_last_error()

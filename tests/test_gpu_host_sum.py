"""pipck_host_sum (include/pipck.h; k_exact_chain and k_resident in
pip_amd/csrc/pipck_host.hip) against tests/host_sum_reference.py, pip's loop in
plain integers, in all five per-call modes: staged (0), zero-copy (1), auto (2),
resident (3) and resident with a device-memory doorbell (4).

Every test drives the C entry point through ctypes on a context of its own, so
the staging buffer and the resident block start from a known state.  Before a
call *out holds a poison word; after it the status is PIPCK_OK and *out is
chain_sum() of the same segments -- the table of host_sum_reference, which
tests/test_host_sum_reference.py pins to pip on the CPU and shows to contain
wrapping inputs for every summing loop."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pip_amd import _lib, engine  # noqa: E402
from pip_amd import checksum as pc  # noqa: E402
from tests import host_sum_reference as hr  # noqa: E402

MODES = (0, 1, 2, 3, 4)
POISON = 0xA5A5A5A5


@pytest.fixture(scope="module", autouse=True)
def gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    engine.require_gpu()
    yield


@pytest.fixture
def ctx_of():
    """ctx_of(mode): a fresh context in that mode, destroyed when the test ends."""
    lib, made = _lib.load(), []

    def make(mode):
        ctx = C.c_void_p()
        _lib.check("pipck_ctx_create", lib.pipck_ctx_create(-1, C.byref(ctx)))
        made.append(ctx)
        _lib.check("pipck_ctx_zero_copy", lib.pipck_ctx_zero_copy(ctx, mode))
        return ctx

    try:
        yield make
    finally:
        for ctx in made:
            lib.pipck_ctx_destroy(ctx)


def _hsegs(segs):
    """(HSeg array, keep-alive): the segments back to back in one host buffer, so
    they start at odd and even addresses; an empty segment still gets a pointer."""
    blob = b"".join(segs)
    buf = C.create_string_buffer(blob, max(len(blob), 1))
    base, off = C.addressof(buf), 0
    arr = (_lib.HSeg * max(len(segs), 1))()
    for i, s in enumerate(segs):
        arr[i].ptr = base + off
        arr[i].len = len(s)
        off += len(s)
    return arr, buf


def _call(ctx, arr, nseg, init):
    out = C.c_uint32(POISON)
    lib = _lib.load()
    rc = lib.pipck_host_sum(ctx, arr, nseg, init, C.byref(out))
    if rc == _lib.PIPCK_EHIP:  # the device or the runtime failed: nothing more may run on it
        pytest.exit("pipck_host_sum: " + (lib.pipck_last_error() or b"").decode(), returncode=3)
    return rc, out.value


def _run(ctx, mode, cases, want_of):
    """Every case in order on ctx; the failures as (name, mode, rc, want, got)."""
    bad = []
    for c in cases:
        arr, keep = _hsegs(c.segs)
        rc, got = _call(ctx, arr, len(c.segs), c.init)
        want = want_of(c)
        if rc != _lib.PIPCK_OK or got > 0xFFFF or got != want:
            bad.append((c.name, "mode %d" % mode, "rc %d" % rc, "want 0x%04x" % want, "got 0x%08x" % got))
        del keep
    return bad


@pytest.mark.parametrize("cls", hr.CLASSES)
@pytest.mark.parametrize("mode", MODES)
def test_table_class_equals_the_reference(ctx_of, mode, cls):
    cases, want = hr.by_class(cls), hr.expected()
    assert cases
    bad = _run(ctx_of(mode), mode, cases, lambda c: want[c.name])
    assert not bad, (len(bad), len(cases), bad[:8])


@pytest.mark.parametrize("mode", MODES)
def test_stale_staging_bytes_stay_out_of_every_sum(ctx_of, mode):
    """The ordered stale sequence on one context: 0xFF-filled calls, then short
    all-zero calls whose 16-byte padding still holds that 0xFF; the 1.5 MiB call
    outgrows the staging buffer (in modes 3 and 4 it halts the resident block,
    which restarts on the new buffer for the calls after it)."""
    seq = hr.stale_sequence()
    bad = _run(ctx_of(mode), mode, seq, lambda c: hr.chain_sum(c.segs, c.init))
    assert not bad, (len(bad), len(seq), bad[:8])


@pytest.mark.parametrize("mode", MODES)
def test_threshold_calls_in_either_order(ctx_of, mode):
    """A first call just over 68 KiB of staged bytes on a fresh context (in modes
    3 and 4 the resident block has not started yet), then the call of exactly
    68 KiB, then over again: the answer does not depend on which path the
    neighbouring call took."""
    by_name = {c.name: c for c in hr.by_class("threshold")}
    want = hr.expected()
    for nseg in (1, 2):
        at = next(c for n, c in by_name.items() if n.startswith("threshold_at_") and len(c.segs) == nseg)
        over = next(c for n, c in by_name.items() if n.startswith("threshold_over_") and len(c.segs) == nseg)
        bad = _run(ctx_of(mode), mode, [over, at, over, at], lambda c: want[c.name])
        assert not bad, bad


@pytest.mark.parametrize("mode", (1, 3))
@pytest.mark.parametrize("fam", (4, 6))
def test_python_chain_wrappers_on_long_chains(oracle, mode, fam):
    """pip_inet_checksum_buf / pip_inet6_checksum_buf of pip_amd.checksum over
    chains of 6, 64, 65 and 130 segments with odd middle lengths, against the
    oracle's restatement of pip's chain functions."""
    import numpy as np

    rng = np.random.default_rng(100 * fam + mode)
    alen = 4 if fam == 4 else 16
    fn = pc.pip_inet_checksum_buf if fam == 4 else pc.pip_inet6_checksum_buf
    ref = oracle.inet_checksum_chain if fam == 4 else oracle.inet6_checksum_chain
    pc.set_zero_copy(mode)
    try:
        for nseg in (6, 64, 65, 130):
            lens = [20] + [int(rng.choice([1, 3, 7, 33, 255, 301])) for _ in range(nseg - 2)] + [int(rng.integers(0, 64))]
            chain = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
            for proto in (6, 17, 255):
                src = rng.integers(0, 256, alen, dtype=np.uint8).tobytes()
                dst = rng.integers(0, 256, alen, dtype=np.uint8).tobytes()
                assert fn(chain, proto, src, dst) == ref(chain, proto, src, dst), (nseg, mode, fam, proto, lens)
    finally:
        pc.set_zero_copy(2)


@pytest.mark.parametrize("mode", MODES)
def test_argument_checks(ctx_of, mode):
    lib, ctx = _lib.load(), ctx_of(mode)
    data = C.create_string_buffer(b"\x12\x34\x56\x78", 4)
    one = (_lib.HSeg * 1)()
    one[0].ptr, one[0].len = C.addressof(data), 4
    out = C.c_uint32(POISON)
    assert lib.pipck_host_sum(None, one, 1, 0, C.byref(out)) == _lib.PIPCK_EINVAL  # null context
    assert out.value == POISON
    assert lib.pipck_host_sum(ctx, one, 1, 0, None) == _lib.PIPCK_EINVAL  # null out
    assert lib.pipck_host_sum(ctx, None, 1, 0, C.byref(out)) == _lib.PIPCK_EINVAL  # no segments, nseg > 0
    assert out.value == POISON
    null = (_lib.HSeg * 3)()
    for i in (0, 2):
        null[i].ptr, null[i].len = C.addressof(data), 4
    null[1].ptr, null[1].len = None, 4  # a null segment with a length
    assert lib.pipck_host_sum(ctx, null, 3, 0, C.byref(out)) == _lib.PIPCK_EINVAL
    assert out.value == POISON
    # a null segment of length 0 is an empty segment, wherever it stands
    null[1].len = 0
    assert _call(ctx, null, 3, 7) == (_lib.PIPCK_OK, hr.chain_sum([data.raw, b"", data.raw], 7))
    null[0].ptr, null[0].len = None, 0
    assert _call(ctx, null, 3, 0xFFFFFFFF) == (_lib.PIPCK_OK, hr.chain_sum([b"", b"", data.raw], 0xFFFFFFFF))
    assert _call(ctx, None, 0, 0xFFFF0001) == (_lib.PIPCK_OK, hr.chain_sum([], 0xFFFF0001))  # no segments at all
    # a mode outside 0..4 is refused and the mode in force stays: the next calls still answer
    for m in (-1, 5):
        assert lib.pipck_ctx_zero_copy(ctx, m) == _lib.PIPCK_EINVAL
        assert _call(ctx, one, 1, 0xFFFFFFFF) == (_lib.PIPCK_OK, hr.chain_sum([data.raw], 0xFFFFFFFF))
    assert lib.pipck_ctx_zero_copy(None, 2) == _lib.PIPCK_EINVAL

"""CPU: the layout of the internal tuning words is written down three times --
the constants in pip_amd/csrc/pipck_tune.hpp (the one that the library is built
from), the tables in pipck_testing.h and TUNE_BITS in pip_amd/engine.py.  This
holds the other two to the header."""
import re
from pathlib import Path

from pip_amd import engine

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "pip_amd" / "csrc"

# engine.tune keyword -> the C++ constant(s) it sets.  k_hdr reads bits 29-31 under names of its own.
KEYWORD_CONSTANTS = {
    "plain_loads": ["kPlainLoads"], "nt_loads": ["kNtLoads"], "flat": ["kNoFlat"], "xcd_groups": ["kXcdGroups"],
    "packed_tiles": ["kNoPackedTiles"], "wide_blocks": ["kWideBlocks"], "small": ["kNoSmall"],
    "flat_small": ["kNoFlatSmall"], "tiny_tiles": ["kNoTinyTiles"], "flat_tiny": ["kNoFlatTiny"],
    "force_flat_tiny": ["kForceFlatTiny"], "packed_marks_only": ["kPackedMarksOnly"], "trace": ["kTrace"],
    "loads_only": ["kLoadsOnly"], "no_task_end": ["kNoTaskEnd"], "end_no_store": ["kEndNoStore"],
    "alt_flat_schedule": ["kAltSchedule"], "plain_result_stores": ["kPlainResultStores", "kHdrPlainStores"],
    "wave_stores": ["kFlatWaveStores", "kHdrNtStores"], "packed_no_align": ["kPackedNoAlign"],
    "free_run": ["kFlatFreeRun", "kHdrNarrowStores"],
}
FIELD_CONSTANTS = {"rows_per_task": ("kRowsShift", "kRowsField"),
                   "small_k_log": ("kSmallDepthShift", "kSmallDepthField")}
RING_CONSTANTS = {"ring_own_slots": "kRingOwnSlots", "ring_all_coop": "kRingAllCoop"}
PROBE_CONSTANTS = {"hdr_in_place": "kProbeHdrInPlace"}
KERNEL_PRIVATE = {"kHdrInPlace"}  # set by a launch function in the kernel's own word, never by pipck_tune


def header_words() -> dict[str, dict[str, int]]:
    """{word: {constant: value}} from the `constexpr uint32_t k... = expr;` lines between `// @word` markers."""
    words: dict[str, dict[str, int]] = {}
    known: dict[str, int] = {}
    word = None
    for line in (CSRC / "pipck_tune.hpp").read_text().splitlines():
        m = re.match(r"// @word (\w+)", line)
        if m:
            word = None if m.group(1) == "end" else m.group(1)
            continue
        m = re.match(r"constexpr uint32_t (k\w+) = ([^;]+);", line)
        if m and word:
            expr = re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)u\b", r"\1", m.group(2))
            assert re.fullmatch(r"[\w\s|<>()]+", expr), line
            known[m.group(1)] = eval(expr, {"__builtins__": {}}, dict(known)) & 0xFFFFFFFF
            words.setdefault(word, {})[m.group(1)] = known[m.group(1)]
    return words


def test_engine_tune_bits_equal_the_header():
    w = header_words()
    flags = w["flags"]
    single = {**engine.TUNE_BITS, **engine.TUNE_INVERTED_BITS}
    assert sorted(single) == sorted(KEYWORD_CONSTANTS)
    for kw, bit in single.items():
        for name in KEYWORD_CONSTANTS[kw]:
            assert flags[name] == 1 << bit, (kw, name)
    assert sorted(engine.TUNE_FIELDS) == sorted(FIELD_CONSTANTS)
    for kw, (shift, width) in engine.TUNE_FIELDS.items():
        cshift, cfield = FIELD_CONSTANTS[kw]
        assert flags[cshift] == shift and flags[cfield] == ((1 << width) - 1) << shift, kw
    for kw, bit in engine.TUNE_RING_BITS.items():
        assert w["ring"][RING_CONSTANTS[kw]] == 1 << bit, kw
    assert engine.TUNE_RING_ADAPT == {None: 0, False: w["ring"]["kRingNoAdapt"], True: w["ring"]["kRingAdaptAll"]}
    for kw, bit in engine.TUNE_PROBE_BITS.items():
        assert w["probes"][PROBE_CONSTANTS[kw]] == 1 << bit, kw
    assert w["lanes"] == {"kWaveArm": 256}


def test_every_header_constant_has_a_keyword_or_is_kernel_private():
    w = header_words()
    named = {n for names in KEYWORD_CONSTANTS.values() for n in names}
    named |= {n for pair in FIELD_CONSTANTS.values() for n in pair}
    assert set(w["flags"]) == named, set(w["flags"]) ^ named
    assert set(w["private"]) == KERNEL_PRIVATE
    assert set(w["ring"]) == set(RING_CONSTANTS.values()) | {"kRingNoAdapt", "kRingAdaptAll"}
    assert set(w["probes"]) == set(PROBE_CONSTANTS.values())
    # a keyword of tune() that sets a flag is in one of the tables, and the tables name only keywords
    import inspect

    params = set(inspect.signature(engine.tune).parameters)
    tabled = (set(engine.TUNE_BITS) | set(engine.TUNE_INVERTED_BITS) | set(engine.TUNE_FIELDS)
              | set(engine.TUNE_RING_BITS) | set(engine.TUNE_PROBE_BITS))
    assert tabled <= params
    assert params - tabled == {"lanes_per_packet", "loads_per_lane", "blocks", "ring_adapt"}


def test_no_word_of_the_header_holds_two_constants_on_one_bit_unless_stated():
    """Inside the flags word only bits 29-31 carry several names (k_flat / k_packed / k_hdr read them
    differently, pipck_tune.hpp's masks section); every other bit and field has one."""
    flags = {n: v for n, v in header_words()["flags"].items() if not n.endswith("Shift")}
    for a, va in flags.items():
        for b, vb in flags.items():
            if a < b and va & vb:
                assert va == vb and va in (1 << 29, 1 << 30, 1 << 31), (a, b)


def test_testing_header_tables_name_every_constant():
    text = (CSRC / "pipck_testing.h").read_text()
    w = header_words()
    for word in ("lanes", "flags", "private", "probes", "ring"):
        for name, value in w[word].items():
            assert re.search(rf"\b{name}\b", text), name
    # and the flag table's bit column agrees with the constant
    for name, value in {**w["flags"], **w["private"]}.items():
        if name.endswith("Shift"):
            continue
        m = re.search(rf"^ \*\s+(\d+)(?:\.\.(\d+))?\s+{name}\b", text, flags=re.M)
        assert m, name
        lo, hi = int(m.group(1)), int(m.group(2) or m.group(1))
        assert value == ((1 << (hi - lo + 1)) - 1) << lo, name

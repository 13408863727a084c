"""The 2-byte layout of a row of the windowed blocked form of K (csrc/kbw_plan.h: kbw_halfword_pos, through dkmc_debug_kbw_halfword_pos): where
k_kbw_assemble<CB, 2> puts entry e of a row padded to 32 or 64 entries, in 16-bit words from the start of the row.  The product gives a row 4 lanes;
with 4-byte words lane l holds ints 4l..4l+3 and 16+4l..16+4l+3 (wide rows: 32+4l.. and 48+4l.. too) in x[0..7] (x[8..15]).  With 16-bit words one
16-byte load per lane has to deliver exactly those entries in those slots: chunk l (eight words) of the row, and chunk 4 + l for a wide row's second
eight.  Also: the new exports as include/ declares them and lib.py binds them (no GPU needed)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from devicekmc_amd import lib
    return lib.load()


@pytest.mark.parametrize("width", [32, 64])
def test_position_map_is_a_permutation(L, width):
    pos = [L.dkmc_debug_kbw_halfword_pos(width, e) for e in range(width)]
    assert sorted(pos) == list(range(width)), pos


@pytest.mark.parametrize("width", [32, 64])
def test_chunk_of_a_lane_holds_its_entries_in_slot_order(L, width):
    entry_at = {L.dkmc_debug_kbw_halfword_pos(width, e): e for e in range(width)}
    for l in range(4):
        first = [entry_at[8 * l + k] for k in range(8)]                       # what lane l's first 16-byte load delivers: x[0..7]
        assert first == [4 * l + u for u in range(4)] + [16 + 4 * l + u for u in range(4)], (l, first)
        if width == 64:
            second = [entry_at[8 * (4 + l) + k] for k in range(8)]            # the wide row's second load: x[8..15]
            assert second == [32 + 4 * l + u for u in range(4)] + [48 + 4 * l + u for u in range(4)], (l, second)


def test_outside_the_row(L):
    for width, e in ((32, -1), (32, 32), (64, 64), (64, -5), (16, 0), (48, 3), (0, 0), (128, 5)):
        assert L.dkmc_debug_kbw_halfword_pos(width, e) == -1, (width, e)


def test_new_exports_declared_and_bound():
    """Signatures of the exports this layout comes with: public switch in devicekmc_hip.h, the two aids in devicekmc_hip_debug.h, lib.py binds them so."""
    from devicekmc_amd import lib
    pub = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "devicekmc_hip.h")).read(), flags=re.S)
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "devicekmc_hip_debug.h")).read(), flags=re.S)
    assert re.search(r"\bvoid\s+dkmc_set_k_window_word_bytes\s*\(\s*int\s+\w+\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_get_k_window_word_bytes\s*\(\s*void\s*\)\s*;", pub)
    assert re.search(r"\bint\s+dkmc_kcg_form_words\s*\(\s*dkmc_gpubuf\s*\*\s*\w+\s*,\s*long long\s*\*\s*\w+\s*\)\s*;", dbg)
    assert re.search(r"\bint\s+dkmc_debug_kbw_halfword_pos\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*\)\s*;", dbg)
    assert "dkmc_kcg_form_words" not in pub and "dkmc_debug_kbw_halfword_pos" not in pub
    S = lib.SYMBOLS
    assert S["dkmc_set_k_window_word_bytes"] == (None, [C.c_int])
    assert S["dkmc_get_k_window_word_bytes"] == (C.c_int, [])
    assert S["dkmc_kcg_form_words"] == (C.c_int, [C.POINTER(lib.dkmc_gpubuf), C.POINTER(C.c_longlong)])
    assert S["dkmc_debug_kbw_halfword_pos"] == (C.c_int, [C.c_int, C.c_int])
    assert S["dkmc_kcg_form_info"] == (C.c_int, [C.POINTER(lib.dkmc_gpubuf), C.POINTER(C.c_longlong)])      # nine fields, unchanged


def test_switch_default_and_clamp(L):
    """The switch lives in the engine (no device needed): 4 by default, 2 selects the 16-bit words, anything else 4."""
    assert L.dkmc_get_k_window_word_bytes() == 4
    try:
        for given, kept in ((2, 2), (4, 4), (0, 4), (3, 4), (16, 4), (-2, 4), (2, 2)):
            L.dkmc_set_k_window_word_bytes(given)
            assert L.dkmc_get_k_window_word_bytes() == kept, (given, kept)
    finally:
        L.dkmc_set_k_window_word_bytes(4)

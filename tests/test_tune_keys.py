"""CPU-only contract of lmg_tune_set / lmg_tune_get: every key's default, the values it accepts and the ones it
refuses, the one alias, the answers to keys that do not exist, and that include/lmg.h documents every key."""
import os
import re

import pytest

from conftest import ROOT
from learnmultigrid_amd import _lib

INT_MAX = 2**31 - 1
ERR_ARG = -1

# key -> (default, rule); a rule is an inclusive range (lo, hi) or a list of the only values accepted
KEYS = {
    "sweep_variant": (0, (0, 6)),
    "pcsr_ju": (0, [0, 1, 3, 5, 101, 102]),
    "rpat_variant": (0, (0, 4)),                 # (>= 1000: the alias, tested on its own)
    "rpat_nt_rows": (8388608, (1, INT_MAX)),
    "stencil_nt_rows": (8388608, (1, INT_MAX)),
    "stencil_wgs_per_cu": (0, (0, 8)),
    "fused_seg_lines": (0, (0, INT_MAX)),
    "fused_seg_min_lines": (0, (0, INT_MAX)),
    "fused_seg_max_lines": (INT_MAX, (0, INT_MAX)),
    "fused_seg_lines_prol": (0, (0, INT_MAX)),
    "fused_seg_lines_rest": (0, (0, INT_MAX)),
    "fused_pf": (0, [0, 2]),
    "fused_want_waves": (5120, (1, INT_MAX)),
    "fused_want_waves_rest3": (2700, (1, INT_MAX)),
    "fused_floor_halos": (4, (1, INT_MAX)),
    "fused_balance": (1, [0, 1]),
    "fused_fast": (1, [0, 1]),
    "fused_slow_pct": (55, (10, 100)),
    "tile_rows": (16, [0, 16, 32]),
    "tile_rows_big": (0, [0, 16, 32]),
    "tile_big_lines": (600, (0, INT_MAX)),
    "tile_prol_wide_lines": (768, (0, INT_MAX)),
    "tile_prol_wide_lines_hx": (1 << 30, (0, INT_MAX)),
    "tile_turnaround_rows": (0, [0, 32, 64]),
    "tile_hot_transfers": (1, [0, 1]),
    "dia_rows": (0, [0, 32, 64]),
    "sell_nt": (-1, (-1, 1)),
    "sell_ju": (0, [0, 5, 7, 8, 10]),
    "gsw_max_sweeps": (4, (1, 4)),
    "gsw_multi_max_rows": (8000000, (0, INT_MAX)),
    "gsw_lds": (-1, (-1, 1)),
    "gsw_lds9": (1, [0, 1]),
    "gsw_lds_multi": (1, [0, 1]),
    "gs_single_max": (2048, (1, INT_MAX)),
}


def accepted(rule):
    if isinstance(rule, list):
        return list(rule)
    lo, hi = rule
    return sorted({lo, min(lo + 1, hi), (lo + hi) // 2, hi})


def refused(rule):
    """One value below and one above the rule (where an int has room for one), and for a list every gap in it."""
    if isinstance(rule, list):
        out = [min(rule) - 1, max(rule) + 1]
        out += [v for v in range(min(rule), max(rule)) if v not in rule and (v - 1 in rule or v + 1 in rule)]
        return out
    lo, hi = rule
    return [lo - 1] + ([hi + 1] if hi < INT_MAX else [])


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_the_table_has_every_key():
    assert len(KEYS) == 34


@pytest.mark.parametrize("key", sorted(KEYS))
def test_default(L, key):
    assert L.lmg_tune_get(key.encode()) == KEYS[key][0]


@pytest.mark.parametrize("key", sorted(KEYS))
def test_accepted_values_read_back(L, key):
    default, rule = KEYS[key]
    kb = key.encode()
    try:
        for v in accepted(rule):
            assert L.lmg_tune_set(kb, v) == 0, (key, v)
            assert L.lmg_tune_get(kb) == v, (key, v)
    finally:
        assert L.lmg_tune_set(kb, default) == 0


@pytest.mark.parametrize("key", sorted(KEYS))
def test_refused_values_change_nothing(L, key):
    default, rule = KEYS[key]
    kb = key.encode()
    keep = accepted(rule)[-1]
    try:
        assert L.lmg_tune_set(kb, keep) == 0
        bad = refused(rule)
        assert len(bad) >= (1 if not isinstance(rule, list) and rule[1] == INT_MAX else 2)
        for v in bad:
            assert L.lmg_tune_set(kb, v) == ERR_ARG, (key, v)
            assert L.lmg_tune_get(kb) == keep, (key, v)
    finally:
        assert L.lmg_tune_set(kb, default) == 0


def test_rpat_variant_from_1000_sets_the_nontemporal_threshold(L):
    try:
        assert L.lmg_tune_set(b"rpat_variant", 3) == 0
        for v in (1000, 123456, INT_MAX):
            assert L.lmg_tune_set(b"rpat_variant", v) == 0
            assert L.lmg_tune_get(b"rpat_nt_rows") == v
            assert L.lmg_tune_get(b"rpat_variant") == 3
        for v in (5, 999, -1):
            assert L.lmg_tune_set(b"rpat_variant", v) == ERR_ARG
            assert L.lmg_tune_get(b"rpat_nt_rows") == INT_MAX
            assert L.lmg_tune_get(b"rpat_variant") == 3
    finally:
        assert L.lmg_tune_set(b"rpat_variant", KEYS["rpat_variant"][0]) == 0
        assert L.lmg_tune_set(b"rpat_nt_rows", KEYS["rpat_nt_rows"][0]) == 0


@pytest.mark.parametrize("key", ["", "nonsense", "tile_", "fused_", "stencil_", "dia_", "sell_", "gsw_", "gs_", "tile_rowsx",
                                 "tile_rows_bigx", "tile_row", "tile_prol_wide_lines_h", "tile_prol_wide_lines_hxx",
                                 "fused_seg_lines_", "fused_seg_lines_pro", "fused_seg_lines_post", "fused_b", "fused_f",
                                 "Tile_rows", " tile_rows", "gsw_lds_", "gsw_lds90", "rpat_variantx", "sweep_varian"])
def test_unknown_keys(L, key):
    before = {k: L.lmg_tune_get(k.encode()) for k in KEYS}
    assert L.lmg_tune_get(key.encode()) == ERR_ARG
    assert L.lmg_tune_set(key.encode(), 0) == ERR_ARG
    assert L.lmg_tune_set(key.encode(), 1) == ERR_ARG
    assert {k: L.lmg_tune_get(k.encode()) for k in KEYS} == before


def test_null_key(L):
    assert L.lmg_tune_get(None) == ERR_ARG
    assert L.lmg_tune_set(None, 0) == ERR_ARG


def test_every_key_is_documented_in_the_header():
    txt = open(os.path.join(ROOT, "include", "lmg.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int lmg_tune_set\(", txt, flags=re.S)
    assert m, "no comment in front of lmg_tune_set"
    documented = set(re.findall(r'"([a-z0-9_]+)"', m.group(1)))
    assert set(KEYS) <= documented, sorted(set(KEYS) - documented)
    assert documented <= set(KEYS), sorted(documented - set(KEYS))

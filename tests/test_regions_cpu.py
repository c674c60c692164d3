"""vsc_regions on the host, no device: the new symbols are declared, exported and bound; vsc_regions_contains equals a brute-force
test of every (contig, position) under both rules - random intervals and hand-made edge cases; the class table uses all three of
its classes; validation; an empty annotation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
from regions_cases import EXPECT, HAND_MADE, LENS, annotation, brute_force, random_intervals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vsc_regions_build", "vsc_regions_free", "vsc_regions_contains", "vsc_regions_info", "vsc_search_summary_regions",
       "vsc_search_select_regions", "vsc_multi_search_summary_regions", "vsc_multi_search_select_regions"]


@pytest.fixture(scope="module")
def packed():
    return va.PackedGenome.from_sequences(["A" * n for n in LENS])


@pytest.fixture(scope="module")
def truth():
    return brute_force(annotation())


def test_region_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(vsc_[a-z0-9_]+)\s*\(", text))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in bound and hasattr(L, name), name
    for word in ("vsc_interval", "vsc_regions_stats", "vsc_region_filter", "VSC_REGION_OVERLAP 0", "VSC_REGION_INSIDE 1",
                 "VSC_REGION_KEEP 0", "VSC_REGION_DROP 1"):
        assert word in text, word
    assert int(re.search(r"#define\s+VSC_ABI_VERSION\s+(\d+)", text).group(1)) == 5
    assert _lib.INTERVAL_DTYPE.itemsize == 16 and C.sizeof(_lib.RegionFilter) == 16 and C.sizeof(_lib.RegionsStats) == 40


@pytest.mark.parametrize("rule", ["overlap", "inside"])
def test_contains_equals_brute_force_everywhere(packed, truth, rule):
    reg = va.Regions(packed, annotation(), rule=rule)
    col = 0 if rule == "overlap" else 1
    for (c, pos), want in EXPECT.items():  # the hand-made cases, against expectations written down by hand ...
        assert reg.contains(c, pos) == bool(want[col]), (rule, c, pos)
        assert bool(truth[rule][c][pos]) == bool(want[col]), (rule, c, pos)
    for c, n in enumerate(LENS):           # ... and every position against the brute force
        got = np.array([reg.contains(c, p) for p in range(n)], dtype=bool)
        bad = np.flatnonzero(got != truth[rule][c])
        assert len(bad) == 0, (rule, c, bad[:10])
        assert not reg.contains(c, n) and not reg.contains(c, 2 ** 32 - 1)
    assert not reg.contains(len(LENS), 0)
    info = reg.info()
    assert info["intervals"] == 400 + len(HAND_MADE) - 1 and info["rule"] == col  # (the empty interval is dropped)
    # both sides of the hand-made windows are there, under either rule
    assert truth[rule][0].any() and not truth[rule][0].all()
    reg.close()


@pytest.mark.parametrize("rule", ["overlap", "inside"])
def test_class_table_uses_all_three_classes(packed, rule):
    reg = va.Regions(packed, annotation(), rule=rule)
    info = reg.info()
    reg.close()
    b = info["block_bases"]
    assert b >= 1 and b & (b - 1) == 0
    total = int(packed.contigs["offset"][-1]) + LENS[-1]
    assert info["blocks_out"] + info["blocks_in"] + info["blocks_mixed"] == (total + b - 1) // b
    assert info["blocks_out"] > 0 and info["blocks_in"] > 0 and info["blocks_mixed"] > 0, info


def test_an_order_free_input(packed):
    """The same intervals in another order, and with every interval given twice: the same answers."""
    iv = annotation()
    a = va.Regions(packed, iv, rule="inside")
    b = va.Regions(packed, sorted(iv) + iv[::-1], rule="inside")
    for c, n in enumerate(LENS):
        assert [a.contains(c, p) for p in range(0, n, 7)] == [b.contains(c, p) for p in range(0, n, 7)]
    a.close()
    b.close()


def test_validation_errors(packed):
    def build(iv, rule=0, reserved=0):
        arr = np.zeros(len(iv), dtype=_lib.INTERVAL_DTYPE)
        for i, (c, s, e) in enumerate(iv):
            arr[i] = (c, s, e, reserved)
        h = C.c_void_p()
        contigs = np.ascontiguousarray(packed.contigs)
        rc = va.lib().vsc_regions_build(_lib.ptr(contigs), len(contigs), _lib.ptr(arr), len(arr), rule, C.byref(h))
        if rc == 0:
            va.lib().vsc_regions_free(h)
        else:
            assert not h.value
        return rc

    assert build([(0, 10, 20)]) == 0
    assert build([(0, 10, 10)]) == 0                  # empty: dropped, not an error
    assert build([(3, 10, 20)]) == -22                # contig >= n_contigs
    assert build([(0, 10, 20), (0, 21, 20)]) == -22   # start > end
    assert build([(0, 10, 20)], reserved=1) == -22
    assert build([(0, 10, 20)], rule=2) == -22
    with pytest.raises(va.VarscotError) as e:
        va.Regions(packed, [(0, 5, 4)])
    assert e.value.code == -22
    with pytest.raises(ValueError):
        va.Regions(packed, [(0, 1, 2)], rule="near")
    assert va.lib().vsc_regions_contains(None, 0, 0) == 0 and va.lib().vsc_regions_info(None, None) == -22
    va.lib().vsc_regions_free(None)


@pytest.mark.parametrize("rule", ["overlap", "inside"])
def test_no_intervals_nothing_is_in(packed, rule):
    for iv in ([], [(1, 700, 700)], [(0, 14000, 14010)]):  # none, one empty, one wholly beyond its contig
        reg = va.Regions(packed, iv, rule=rule)
        assert not any(reg.contains(c, p) for c, n in enumerate(LENS) for p in range(0, n, 3))
        info = reg.info()
        assert info["intervals"] == 0 and info["blocks_in"] == 0 and info["blocks_mixed"] == 0 and info["blocks_out"] > 0
        reg.close()


def test_random_intervals_are_what_the_issue_asks_for():
    iv = random_intervals()
    ln = np.array([e - s for _, s, e in iv])
    assert len(iv) == 400 and ln.min() >= 1 and ln.max() <= 3000 and (ln > 1000).any() and (ln < 10).any()

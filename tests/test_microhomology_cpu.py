"""The host side of the microhomology score (vsc_mh_score_text, vsc_mh_scores, the shape): the library's mask form against the
row list of tests/microhomology_cases.py, as integers.  No device is needed."""
import ctypes as C
import math

import numpy as np
import pytest

import microhomology_cases as mc
import varscot_amd as va
from varscot_amd import _lib


@pytest.mark.parametrize("F", mc.FLANKS)
def test_score_text_equals_the_row_list(F):
    families = set()
    for family, text in mc.contexts(F):
        families.add(family)
        assert va.microhomology_text(text) == mc.score(text, F), (family, text)
        assert va.microhomology_text(text, flank=F) == mc.score(text, F)
    assert families >= {"random", "halves", "halves_but_one", "period", "two_letters", "none", "one_row"}


def test_the_families_hold_what_they_are_for():
    for F in mc.FLANKS:
        by = {}
        for family, text in mc.contexts(F):
            by.setdefault(family, []).append((text, mc.score(text, F), mc.rows(text, F)))
        assert all(s == (0, 0) and not r for _, s, r in by["none"])
        # the quirk: the one run of F at d = F is listed as its two rows of F - 1
        for text, _, r in by["halves"]:
            assert sorted(x for x in r if x[1] - x[0] == F) == [(0, F, F - 1), (1, F + 1, F - 1)]
        assert any(max((k for i, j, k in r if j - i == F), default=0) == F - 1 for _, _, r in by["halves_but_one"])
        assert any(0 < max((k for i, j, k in r if j - i == F), default=0) < F - 1 for _, _, r in by["halves_but_one"])
        assert sorted(len(r) for _, _, r in by["one_row"]) == [1, 1, 1]
        assert sum(s[1] == 0 for _, s, _ in by["one_row"]) == 1 and sum(s[1] == s[0] for _, s, _ in by["one_row"]) == 2
    total, oof = mc.score(mc.two_thirds(), 30)
    # 2 : 3 is 666.67 per mille: FILTER keeps it at 666 and drops it at 667 (2000 < 2001), in integers
    assert total > 0 and 3 * oof == 2 * total and mc.keep((total, oof), 0, 666) and not mc.keep((total, oof), 0, 667)
    assert mc.keep((3000, 2001), 0, 667) and not mc.keep((3000, 2000), 0, 667) and mc.keep((0, 0), 0, 0) and not mc.keep((0, 0), 0, 1)


def test_the_table_is_the_formula_and_has_no_tie():
    want = [int(round(round(math.exp(-d / 20.0), 3) * 1000.0)) for d in range(64)]
    assert want[:11] == [1000, 951, 905, 861, 819, 779, 741, 705, 670, 638, 607] and want[-3:] == [47, 45, 43]
    for d in range(1, 64):
        x = 1000.0 * math.exp(-d / 20.0)
        assert abs(x - math.floor(x) - 0.5) >= 0.0047, d
    # the library's table, read off a context with one row of two A/T letters at every deletion length it can have
    for F in (8, 32):
        for d in range(2, 2 * F - 1):
            i = max(0, F - d)
            if i + 2 > F or i + d + 2 > 2 * F:
                continue
            left, right = ["A"] * F, ["C"] * F
            left[i:i + 2] = "TT"
            right[i + d - F:i + d - F + 2] = "TT"
            text = "".join(left + right)
            got = va.microhomology_text(text)
            assert got == mc.score(text, F) and got[0] == 2 * want[d], (F, d)


def test_the_largest_sum_fits():
    largest = max(mc.score(text, F)[0] for F in mc.FLANKS for _, text in mc.contexts(F))
    assert largest == mc.score("G" * 64, 32)[0] == va.microhomology_text("G" * 64)[0]
    assert largest < 4.1e6 < 2 ** 32 - 1


def test_scores_are_one_division_each():
    pairs = [mc.score(text, F) for F in mc.FLANKS for _, text in mc.contexts(F)]
    assert any(s == 0 for s, _ in pairs) and any(0 < o < s for s, o in pairs)
    mh, oof = va.microhomology_scores(np.array(pairs, dtype=np.uint32))
    for (s, o), x, y in zip(pairs, mh, oof):
        assert x == s / 10 and y == (100 * o / s if s else 0.0)
    assert va.microhomology_scores((1098, 732)) == (109.8, 100 * 732 / 1098)
    x, y = va.microhomology_scores((va.MH_UNDEFINED, va.MH_UNDEFINED))
    assert x != x and y != y
    a, b = C.c_double(), C.c_double()
    assert va.lib().vsc_mh_scores(5, 6, C.byref(a), C.byref(b)) == -22  # oof > sum is no pair
    assert va.lib().vsc_mh_scores(5, 5, None, C.byref(b)) == -22


def test_the_published_float_sum_is_the_integers_but_for_rounding():
    n = 0
    for F in mc.FLANKS:
        for _, text in mc.contexts(F):
            total = mc.score(text, F)[0]
            x = mc.published_float(text, F)
            if total:
                n += 1
                assert abs(x - total / 10) <= 1e-9 * (total / 10), text
                assert int(x) in (total // 10, total // 10 - 1)  # only its int() can differ, and only downwards
            else:
                assert x == 0.0
    assert n > 200


def test_shape_refusals():
    for kw in ({"flank": 7}, {"flank": 33}, {"cut": 24}, {"site_len": 15, "cut": 10}, {"site_len": 33}, {"cut": -1}):
        with pytest.raises(ValueError):
            va.MicrohomologyShape(**kw)
    for kw in ({"flank": 8}, {"flank": 32}, {"cut": 0}, {"cut": 23}, {"site_len": 16, "cut": 16}, {"site_len": 32, "cut": 32}):
        s = va.MicrohomologyShape(**kw)._struct()
        assert C.sizeof(s) == 16 and s.reserved == 0
    s, o = C.c_uint32(), C.c_uint32()
    L = va.lib()
    for F in (7, 33, 0, 0xFFFFFFFF):
        assert L.vsc_mh_score_text(b"A" * 66, F, C.byref(s), C.byref(o)) == -22
    assert L.vsc_mh_score_text(b"A" * 15, 8, C.byref(s), C.byref(o)) == -22
    assert L.vsc_mh_score_text(b"A" * 17, 8, C.byref(s), C.byref(o)) == -22
    assert L.vsc_mh_score_text(None, 8, C.byref(s), C.byref(o)) == -22
    assert L.vsc_mh_score_text(b"A" * 16, 8, None, C.byref(o)) == -22
    with pytest.raises(ValueError):
        va.microhomology_text("A" * 17)
    assert C.sizeof(_lib.MhStats) == 64


def test_text_case_and_other_letters():
    rng = np.random.default_rng(4)
    for F in (8, 30):
        text = mc.contexts(F)[0][1]
        want = mc.score(text, F)
        assert want[0] > 0
        assert va.microhomology_text(text.lower()) == want
        mixed = "".join(ch.lower() if rng.integers(0, 2) else ch for ch in text)
        assert va.microhomology_text(mixed) == want
        for ch in "NnRY-*":
            at = int(rng.integers(0, 2 * F))
            assert va.microhomology_text(text[:at] + ch + text[at + 1:]) == (va.MH_UNDEFINED, va.MH_UNDEFINED)
    assert va.MH_UNDEFINED == 0xFFFFFFFF


def test_python_floors_become_integers_once():
    f = va.Genome._mh_args
    shape = va.MicrohomologyShape()
    assert f(None, None, None, 23) is None and f(shape, None, None, 23) == (shape, None, None)
    assert f(shape, 66.7, None, 23) == (shape, 0, 667) and f(shape, None, 109.8, 23) == (shape, 1098, 0)
    assert f(shape, 100, 0, 23) == (shape, 0, 1000)
    for bad in ((None, 50, None), (None, None, 1.0), (shape, 100.1, None), (shape, -1, None), ("x", None, None)):
        with pytest.raises(ValueError):
            f(*bad, 23)
    with pytest.raises(ValueError):
        f(va.MicrohomologyShape(site_len=27), None, None, 23)

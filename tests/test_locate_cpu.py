"""vsc_regions_locate on the host, no device: the label of every window of the three-contig layout under both rules equals the
brute force of the definition (tests/locate_cases.py) and is REGION_NONE exactly where vsc_regions_contains says no; the tie
rules; the annotations that make the lookup walk (a staircase of nested intervals, a whole-contig interval in front of 2 000
short ones); no intervals at all; the new symbols."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
from locate_cases import NONE, brute_labels, staircase, whole_contig
from regions_cases import HAND_MADE, LENS, WINDOW, annotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = ["overlap", "inside"]


@pytest.fixture(scope="module")
def packed():
    return va.PackedGenome.from_sequences(["A" * n for n in LENS])


def located(reg, contig, positions):
    return np.array([reg.locate(contig, int(p)) for p in positions], dtype=np.uint32)


def test_locate_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    assert re.search(r"#define\s+VSC_REGION_NONE\s+0xFFFFFFFFu", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(vsc_[a-z0-9_]+)\s*\(", text))
    bound = {name for name, _, _ in _lib.SYMBOLS}
    L = C.CDLL(_lib.LIB_PATH)
    for name in ("vsc_regions_locate", "vsc_hits_locate", "vsc_guides_locate"):
        assert name in declared and name in bound and hasattr(L, name), name
    assert int(re.search(r"#define\s+VSC_ABI_VERSION\s+(\d+)", text).group(1)) == 5
    assert va.REGION_NONE == NONE == 0xFFFFFFFF


@pytest.mark.parametrize("rule", RULES)
def test_locate_equals_brute_force_everywhere(packed, rule):
    iv = annotation()
    reg = va.Regions(packed, iv, rule=rule)
    for c, n in enumerate(LENS):
        pos = np.arange(n)
        got = located(reg, c, pos)
        want = brute_labels(iv, rule, c, pos)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (rule, c, bad[:10], got[bad[:10]], want[bad[:10]])
        inside = np.array([reg.contains(c, int(p)) for p in pos], dtype=bool)
        assert np.array_equal(got != NONE, inside), (rule, c)  # the invariant, the cut-off windows at the contig's end included
        assert reg.locate(c, n) == NONE and reg.locate(c, 2 ** 32 - 1) == NONE
    assert reg.locate(len(LENS), 0) == NONE
    # the hand-made cases: the short interval nested in the long one wins where the window is in both, the long one elsewhere;
    # the empty interval takes a number but labels nothing, and the numbers after it are not shifted
    at = {case[:3]: i for i, case in enumerate(iv)}
    long_one, short_one = at[(0, 12100, 12600)], at[(0, 12200, 12210)]
    assert reg.locate(0, 12300) == long_one
    assert reg.locate(0, 12205) == (short_one if rule == "overlap" else long_one)
    assert at[(1, 700, 700)] not in set(located(reg, 1, range(LENS[1])).tolist())
    assert reg.locate(2, 0) == at[(2, 0, 40)]
    assert reg.locate(1, 4977) == at[(1, 4900, 9999)]  # clipped to the contig: the last whole window inside it
    assert reg.locate(1, 4999) == (at[(1, 4900, 9999)] if rule == "overlap" else NONE)  # a cut-off window
    assert len(HAND_MADE) == 13
    reg.close()


def test_tie_rules():
    packed = va.PackedGenome.from_sequences(["A" * 1000])
    lens = [1000]
    # the same start, different ends: the smallest end that still qualifies
    iv = [(0, 100, 200), (0, 100, 150), (0, 100, 300)]
    for rule in RULES:
        reg = va.Regions(packed, iv, rule=rule)
        pos = np.arange(1000)
        assert np.array_equal(located(reg, 0, pos), brute_labels(iv, rule, 0, pos, lens))
        assert reg.locate(0, 110) == 1 and reg.locate(0, 160) == 0 and reg.locate(0, 250) == 2
        assert reg.locate(0, 140) == (1 if rule == "overlap" else 0)  # [140, 163) lies inside 100-200, not inside 100-150
        reg.close()
    # exact duplicates: the first one given, wherever the others stand
    iv = [(0, 50, 400), (0, 100, 200), (0, 100, 200), (0, 50, 400), (0, 100, 200)]
    for rule in RULES:
        reg = va.Regions(packed, iv, rule=rule)
        assert reg.locate(0, 120) == 1 and reg.locate(0, 300) == 0
        assert np.array_equal(located(reg, 0, np.arange(1000)), brute_labels(iv, rule, 0, np.arange(1000), lens))
        reg.close()


@pytest.mark.parametrize("rule", RULES)
def test_a_permuted_input_chooses_the_same_interval(packed, rule):
    iv = annotation()
    iv = iv + iv[10:40]  # with exact duplicates
    perm = np.random.default_rng(99).permutation(len(iv))
    iv_p = [iv[i] for i in perm]
    a, b = va.Regions(packed, iv, rule=rule), va.Regions(packed, iv_p, rule=rule)
    for c, n in enumerate(LENS):
        pos = np.arange(0, n, 3)
        la, lb = located(a, c, pos), located(b, c, pos)
        assert np.array_equal(la == NONE, lb == NONE)
        for x, y in zip(la[la != NONE].tolist(), lb[lb != NONE].tolist()):
            assert iv[x] == iv_p[y], (c, x, y)                 # the same interval ...
            assert y == min(j for j in range(len(iv_p)) if iv_p[j] == iv_p[y])  # ... and of its duplicates the first given
        assert np.array_equal(lb, brute_labels(iv_p, rule, c, pos))
    a.close()
    b.close()


@pytest.mark.parametrize("rule", RULES)
def test_a_staircase_of_nested_intervals(packed, rule):
    """40 intervals, starts rising and ends falling: a window near the right edge lies beyond most ends, the lookup climbs
    tens of enclosing intervals."""
    iv = staircase()
    reg = va.Regions(packed, iv, rule=rule)
    pos = np.arange(2500, 3030)
    got = located(reg, 0, pos)
    assert np.array_equal(got, brute_labels(iv, rule, 0, pos))
    assert len(set(got.tolist()) - {NONE}) == 40 and (got == NONE).any()  # every step of the staircase is somebody's label
    pos = np.arange(900, 1500)
    assert np.array_equal(located(reg, 0, pos), brute_labels(iv, rule, 0, pos))
    reg.close()


@pytest.mark.parametrize("rule", RULES)
def test_a_whole_contig_interval_before_2000_short_ones(rule):
    """Windows in the gaps between the short intervals are in the whole-contig one only - it stands 2 000 entries back."""
    length = 90000
    packed = va.PackedGenome.from_sequences(["A" * length])
    iv = whole_contig(length)
    pitch = length // 2000
    reg = va.Regions(packed, iv, rule=rule)
    gaps = np.array([pitch * i + 10 + d for i in range(2000) for d in (0, 5, 11)])  # [p, p + 23) meets no short interval
    assert np.all(located(reg, 0, gaps) == 0)
    pos = np.concatenate([np.arange(0, 3000), np.arange(length - 3000, length)])
    got = located(reg, 0, pos)
    assert np.array_equal(got, brute_labels(iv, rule, 0, pos, [length]))
    if rule == "overlap":
        assert (got > 0).any() and (got == 0).any()
    else:
        assert set(got.tolist()) == {0, NONE}  # (5 bases hold no window; the last 22 starts are cut-off windows)
    reg.close()
    # the same on the three-contig layout, where the short ones stand closer than a window is long
    packed = va.PackedGenome.from_sequences(["A" * n for n in LENS])
    iv = whole_contig(LENS[0], short=3)
    reg = va.Regions(packed, iv, rule=rule)
    pos = np.arange(LENS[0])
    assert np.array_equal(located(reg, 0, pos), brute_labels(iv, rule, 0, pos))
    reg.close()


@pytest.mark.parametrize("rule", RULES)
def test_nothing_to_label(packed, rule):
    for iv in ([], [(1, 700, 700)], [(0, 14000, 14010)]):
        reg = va.Regions(packed, iv, rule=rule)
        assert all(reg.locate(c, p) == NONE for c, n in enumerate(LENS) for p in range(0, n, 3))
        reg.close()
    # one interval shorter than a window: nothing lies inside it, 22 + 10 windows overlap it
    reg = va.Regions(packed, [(0, 300, 310)], rule=rule)
    got = located(reg, 0, np.arange(250, 350))
    if rule == "inside":
        assert np.all(got == NONE)
    else:
        assert np.array_equal(np.flatnonzero(got == 0) + 250, np.arange(300 - WINDOW + 1, 310))
    reg.close()
    assert va.lib().vsc_regions_locate(None, 0, 0) == NONE
    assert va.lib().vsc_hits_locate(None, None, None) == -22 and va.lib().vsc_guides_locate(None, None, None) == -22


def test_guide_summary_refuses_a_stray_region_name_option(tmp_path):
    """-N names the -A interval of a -T hit or the -E interval of a -L guide: without either pair, or with another word, the
    tool stops at its usage check, before it looks for a genome or a device."""
    tool = os.path.join(ROOT, "varscot_amd", "bin", "guide_summary")
    base = [tool, "-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "idx"), "-M", "3"]
    reads, bed = ["-R", str(tmp_path / "r.fa")], str(tmp_path / "a.bed")
    for extra in (reads + ["-N", "name"], reads + ["-A", bed, "-N", "name"], reads + ["-T", str(tmp_path / "t.tsv"), "-N", "coords"],
                  ["-E", bed, "-N", "coords"], reads + ["-A", bed, "-T", str(tmp_path / "t.tsv"), "-N", "gene"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "-N" in r.stderr, (extra, r.stderr)

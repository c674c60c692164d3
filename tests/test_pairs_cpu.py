"""The paired-nickase screen's host side, no device needed: the new entry points are declared, exported and bound, the layouts of
the four structs, vsc_loci_pairs against the brute force of tests/pairs_cases.py (hand-worked loci, random loci in shuffled and
sorted order, PAM-in ranges, ranges that clip at 0, entries that take part in nothing, the count-only call, a short capacity,
invalid parameters), nickase_delta, and guide_summary's -j / -J argument checks (all made before a device is opened)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import pairs_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("VSC_TEST_BIN") or os.path.join(ROOT, "varscot_amd", "bin")
NEW = ["vsc_loci_pairs", "vsc_guides_pairs", "vsc_hits_pairs"]


def loci_of(rows):
    out = np.zeros(len(rows), dtype=va.LOCUS_DTYPE)
    for i, (c, p, s) in enumerate(rows):
        out[i] = (c, p, s, 0)
    return out


def raw_pairs(loci, delta, capacity=None, count_only=False, reserved=(0, 0)):
    """vsc_loci_pairs as it is: (status, n_pairs, the pairs buffer)."""
    p = _lib.PairParams()
    p.delta_min, p.delta_max = delta
    p.reserved[0], p.reserved[1] = reserved
    n = C.c_uint64(12345)
    buf = None if count_only else np.full((capacity, 2), 0xEEEEEEEE, dtype=np.uint32)
    rc = va.lib().vsc_loci_pairs(_lib.ptr(loci), len(loci), C.byref(p), _lib.ptr(buf), 0 if count_only else capacity, C.byref(n))
    return rc, int(n.value), buf


def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in bound, name
        assert hasattr(L, name), name
        assert getattr(va.lib(), name).argtypes is not None
    assert int(re.search(r"#define\s+VSC_ABI_VERSION\s+(\d+)", text).group(1)) == 5  # additive: the version stays
    assert va.lib().vsc_abi_version() == 5
    # the header gives the definition and says what vsc_ctx_timing reports
    about = text[text.index("Paired-nickase screen"):text.index("vsc_loci_pairs(const")]
    assert "delta = pos(the '+' window) - pos(the '-' window)" in about and "vsc_ctx_timing" in about


def test_struct_layouts(tmp_path):
    sizes = {"vsc_pair_params": (_lib.PairParams, 16), "vsc_guide_pair": (_lib.GuidePair, 8),
             "vsc_pair_summary": (_lib.PairSummary, 224), "vsc_pair_site": (_lib.PairSite, 16)}
    for name, (cls, size) in sizes.items():
        assert C.sizeof(cls) == size, name
    offsets = {
        "vsc_pair_params": [("delta_min", 0), ("delta_max", 4), ("reserved", 8)],
        "vsc_guide_pair": [("a", 0), ("b", 4)],
        "vsc_pair_summary": [("sites", 0), ("nm_sum", 8), ("nm_max", 144), ("on_target", 216), ("reserved", 220)],
        "vsc_pair_site": [("pair", 0), ("a_rec", 4), ("b_rec", 8), ("delta", 12)],
    }
    for name, (cls, _) in sizes.items():
        assert [(n, getattr(cls, n).offset) for n, _ in cls._fields_] == offsets[name], name
    for dt, cls, mine in ((_lib.PAIR_SUMMARY_DTYPE, _lib.PairSummary, pc.PAIR_SUMMARY), (_lib.PAIR_SITE_DTYPE, _lib.PairSite, pc.PAIR_SITE)):
        assert dt == mine and dt.itemsize == C.sizeof(cls)
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(cls, n).offset) for n, _ in cls._fields_]
    assert va.PairParams is _lib.PairParams and va.PAIR_SITE_DTYPE is _lib.PAIR_SITE_DTYPE
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:
        lines = ['#include <stddef.h>', '#include "varscot_hip.h"']
        for name, (_, size) in sizes.items():
            lines.append('_Static_assert(sizeof(%s) == %d, "size");' % (name, size))
            for field, off in offsets[name]:
                lines.append('_Static_assert(offsetof(%s, %s) == %d, "offset");' % (name, field, off))
        src = tmp_path / "layout.c"
        src.write_text("\n".join(lines) + "\n")
        r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr


def test_nickase_delta():
    assert va.nickase_delta(-4, 20) == (19, 43)
    assert va.nickase_delta(0, 0) == (23, 23)
    assert va.nickase_delta(-60, -30) == (-37, -7)  # PAM-in: the '-' window lies to the right


def test_hand_worked_loci():
    # contig 0: '-' at 100; '+' at 119 (delta 19), 120 (20), 143 (43), 144 (44), a '-' at 120 (same strand), and on contig 1 a
    # '+' at 120; the last entry repeats the '+' at 120: simply another entry
    loci = loci_of([(0, 100, 1), (0, 119, 0), (0, 120, 0), (0, 143, 0), (0, 144, 0), (0, 120, 1), (1, 120, 0), (0, 120, 0)])
    # (the '-' at 120 has the '+' windows at 143 and 144 to its right: delta 23 and 24)
    assert va.pair_loci(loci, (20, 43)).tolist() == [[0, 2], [0, 3], [0, 7], [5, 3], [5, 4]]
    assert va.pair_loci(loci, (19, 44)).tolist() == [[0, 1], [0, 2], [0, 3], [0, 4], [0, 7], [5, 3], [5, 4]]
    assert va.pair_loci(loci, (25, 43)).tolist() == [[0, 3]]
    # a range that reaches to the left (PAM-in) finds the '+' windows at or before the '-' window
    assert va.pair_loci(loci, (-1, 0)).tolist() == [[5, 1], [5, 2], [5, 7]]
    assert va.pair_loci(loci, (0, 0)).tolist() == [[5, 2], [5, 7]]
    assert va.pair_loci(loci, (200, 300)).shape == (0, 2)
    # the brute force says the same of every case
    for delta in ((20, 43), (19, 44), (25, 43), (-1, 0), (0, 0), (200, 300)):
        assert np.array_equal(va.pair_loci(loci, delta), pc.brute_loci_pairs(loci, delta)), delta
    # (contig, pos, strand) rows are taken as well
    assert va.pair_loci([(0, 100, 1), (0, 130, 0)], (23, 43)).tolist() == [[0, 1]]


def random_loci(seed, n=300):
    rng = np.random.default_rng(seed)
    loci = np.zeros(n, dtype=va.LOCUS_DTYPE)
    loci["contig"] = rng.integers(0, 3, n)
    loci["pos"] = rng.integers(0, 1500, n)  # dense: many partners, equal loci among them
    loci["strand"] = rng.integers(0, 2, n)
    return loci


@pytest.mark.parametrize("delta", [(19, 43), (-40, -7), (-30, 30), (0, 0), (1400, 3000)])
def test_random_loci_shuffled_and_sorted(delta):
    loci = random_loci(3)
    want = pc.brute_loci_pairs(loci, delta)
    assert np.array_equal(va.pair_loci(loci, delta), want)
    assert len(want) or delta == (0, 0) or delta[0] > 1000
    order = np.lexsort((loci["strand"], loci["pos"], loci["contig"]))  # vsc_guides_enumerate's order
    srt = np.ascontiguousarray(loci[order])
    got = va.pair_loci(srt, delta)
    assert np.array_equal(got, pc.brute_loci_pairs(srt, delta))
    assert len(got) == len(want)
    if len(got):
        assert np.all(np.diff(got[:, 0].astype(np.int64) * 2 ** 32 + got[:, 1]) > 0)  # ascending (a, b), no pair twice


def test_ranges_that_clip_and_entries_that_take_part_in_nothing():
    top = 0xFFFFFFFF
    loci = loci_of([(0, 5, 1), (0, 0, 0), (0, 3, 0), (0, 9, 0), (0, top, 0), (0, top - 10, 1), (0, top - 30, 0),
                    (pc.NONE, 5, 1), (pc.NONE, 6, 0), (2, 7, 1), (2, 8, 0)])
    for delta in ((-100, -1), (-5, 4), (-2 ** 30, 2 ** 30), (0, 2 ** 30), (-2 ** 30, 0), (10, 10), (-20, -20)):
        got = va.pair_loci(loci, delta)
        assert np.array_equal(got, pc.brute_loci_pairs(loci, delta)), delta
        assert not np.isin(got, [7, 8]).any()  # contig UINT32_MAX: in no pair, not even with each other
    assert va.pair_loci(loci, (-5, 4)).tolist() == [[0, 1], [0, 2], [0, 3], [9, 10]]
    assert va.pair_loci(loci, (10, 10)).tolist() == [[5, 4]]  # pos + delta = UINT32_MAX exactly


def test_count_only_and_short_capacity():
    loci = random_loci(4)
    want = pc.brute_loci_pairs(loci, (19, 43))
    assert len(want) > 10
    rc, n, _ = raw_pairs(loci, (19, 43), count_only=True)
    assert (rc, n) == (0, len(want))
    rc, n, buf = raw_pairs(loci, (19, 43), capacity=len(want) - 1)
    assert rc == -34 and n == len(want)  # VSC_ERR_RANGE with the count set ...
    assert np.all(buf == 0xEEEEEEEE)      # ... and nothing written
    rc, n, buf = raw_pairs(loci, (19, 43), capacity=len(want) + 3)
    assert (rc, n) == (0, len(want)) and np.array_equal(buf[:n], want) and np.all(buf[n:] == 0xEEEEEEEE)
    rc, n, _ = raw_pairs(loci[:0], (19, 43), count_only=True)
    assert (rc, n) == (0, 0)


def test_invalid_parameters():
    loci = random_loci(5, 20)
    for delta in ((5, 4), (-2 ** 30 - 1, 0), (0, 2 ** 30 + 1), (-2 ** 31, 2 ** 31 - 1)):
        rc, n, _ = raw_pairs(loci, delta, count_only=True)
        assert (rc, n) == (-22, 0), delta
        with pytest.raises(va.VarscotError) as e:
            va.pair_loci(loci, delta)
        assert e.value.code == -22
    assert raw_pairs(loci, (-2 ** 30, 2 ** 30), count_only=True)[0] == 0  # the bounds themselves are allowed
    for reserved in ((1, 0), (0, 1)):
        assert raw_pairs(loci, (0, 10), count_only=True, reserved=reserved)[0] == -22
    p = _lib.PairParams(0, 10)
    n = C.c_uint64()
    assert va.lib().vsc_loci_pairs(None, 3, C.byref(p), None, 0, C.byref(n)) == -22  # loci missing
    assert va.lib().vsc_loci_pairs(_lib.ptr(loci), len(loci), None, None, 0, C.byref(n)) == -22
    assert va.lib().vsc_loci_pairs(_lib.ptr(loci), len(loci), C.byref(p), None, 0, None) == -22
    with pytest.raises(ValueError):
        va.pair_loci(loci, (0, 2 ** 31))


def test_planter_meets_the_guards_the_gpu_tests_rely_on(oracle):
    """The planted genome by the oracle and the brute force alone: both strand assignments, the boundary deltas, a site total
    of the wide range that is no multiple of a wave or a workgroup, the guides that must have no or one hit."""
    pl = pc.planted()
    hits = oracle.search(pl["contigs"], pl["guides"], pc.M, mode=oracle.MODE_PREDICATE)
    g = hits["guide"]
    assert int((g == pc.NOHIT).sum()) == 0 and int((g == pc.NEVER).sum()) == 0 and int((g == pc.ONCE).sum()) == 1
    rows, sites = pc.brute_hits_pairs(hits, pc.PAIRS, pc.DELTA, pl["exclude"])
    assert int(rows["sites"].sum()) >= 20 and rows["on_target"].tolist() == [1, 0, 0, 0, 1, 1]  # (B, A) meets the same locus
    assert rows["sites"][3] == 0 and rows["sites"][0] == rows["sites"][4] == rows["sites"][5] > 0
    assert {pc.DELTA[0], pc.DELTA[1]} <= set(sites[:, 3].tolist())
    assert set(((hits["info"] >> 31)[sites[:, 1]]).tolist()) == {0, 1}
    _, wide = pc.brute_hits_pairs(hits, pc.all_ordered_pairs(), pc.WIDE, pl["exclude"])
    assert len(wide) > 1024 and len(wide) % 64 and len(wide) % 256
    assert np.bincount(wide[:, 1]).max() > 8  # single records with many partners
    # the host pairing over the records' own loci says what the brute force says of pair (A, B) with A on '-'
    strand = hits["info"] >> 31
    keep = ((g == pc.A) & (strand == 1)) | ((g == pc.B) & (strand == 0))
    loci = np.zeros(int(keep.sum()), dtype=va.LOCUS_DTYPE)
    loci["contig"], loci["pos"], loci["strand"] = hits["contig"][keep], hits["pos"][keep], strand[keep]
    plain, plain_sites = pc.brute_hits_pairs(hits, [(pc.A, pc.B)], pc.DELTA)
    minus_a = plain_sites[strand[plain_sites[:, 1]] == 1]
    got = va.pair_loci(loci, pc.DELTA)
    assert 0 < len(minus_a) < plain["sites"][0] and len(got) == len(minus_a)
    back = np.nonzero(keep)[0]
    assert np.array_equal(back[got], minus_a[:, 1:3])


def summary(*args):
    return subprocess.run([os.path.join(BIN, "guide_summary")] + list(args), capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_guide_summary_pair_argument_errors(tmp_path):
    (tmp_path / "g.fa").write_text(">c\n" + "ACGT" * 30 + "\n")
    (tmp_path / "r.fa").write_text(">r\n" + "ACGT" * 5 + "AGG\n")
    (tmp_path / "t.bed").write_text("c\t0\t100\n")
    base = ["-G", str(tmp_path / "g.fa"), "-I", str(tmp_path / "none"), "-M", "3"]
    out = str(tmp_path / "pairs.tsv")
    cases = [
        (["-E", str(tmp_path / "t.bed"), "-J", out], "-j"),                          # -J without -j
        (["-E", str(tmp_path / "t.bed"), "-j", "-4,20"], "-J"),                      # -j without -J
        (["-R", str(tmp_path / "r.fa"), "-J", out, "-j", "-4,20"], "-E or -B"),      # reads have no loci
        (["-E", str(tmp_path / "t.bed"), "-J", out, "-j", "20,-4"], "MIN,MAX"),
        (["-E", str(tmp_path / "t.bed"), "-J", out, "-j", "7"], "MIN,MAX"),
        (["-E", str(tmp_path / "t.bed"), "-J", str(tmp_path / "pairs.bed"), "-j", "-4,20"], ".tsv"),
    ]
    for extra, word in cases:
        r = summary(*(base + extra))
        assert r.returncode != 0, extra
        assert word in r.stderr, (extra, r.stderr)
        assert "Index loaded" not in r.stderr and "no HIP device" not in r.stderr, r.stderr  # refused before any device work
        assert not os.path.exists(out)

"""The per-guide summary's host side, no device needed: CRISPOR's guide-level MIT specificity from fixed-point sums
(vsc_mit_specificity), the summary row layout, and guide_summary's argument checks (all made before a device is opened)."""
import math
import os
import subprocess

import numpy as np

import varscot_amd as va

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("VSC_TEST_BIN") or os.path.join(ROOT, "varscot_amd", "bin")


def test_mit_specificity_reproduces_crispor(golden_dir):
    """CRISPOR's mitSpecScore of the 7 SITE-Seq guides = round(100 / (100 + sum of its off-targets' mitOfftargetScore) * 100)
    (Python 2 round: floor(x + 0.5)), the sum taken in units of 2^-24 as vsc_search_summary accumulates it."""
    lines = open(os.path.join(golden_dir, "crispor_guides.tsv")).read().splitlines()
    assert lines[0].split("\t") == ["guideSeq", "offtargetCount", "mitSpecScore", "mitSumFixed24"]
    rows = [line.split("\t") for line in lines[1:]]
    assert len(rows) == 7
    for seq, count, spec, fixed in rows:
        x = va.mit_specificity(int(fixed))
        assert x == (100.0 / (100.0 + int(fixed) * 2.0 ** -24)) * 100.0
        assert math.floor(x + 0.5) == int(spec), (seq, x, spec)
        assert abs(x - round(x)) > 0.01  # none of them sits near a .5 boundary
    assert va.mit_specificity(0) == 100.0


def test_summary_dtype_layout():
    assert va.SUMMARY_DTYPE.itemsize == 96
    assert va.SUMMARY_DTYPE.names == ("mit_sum", "nm", "mit_ub", "on_target", "reserved")
    assert va.SUMMARY_DTYPE.fields["nm"][0].shape == (9,) and va.SUMMARY_DTYPE.fields["on_target"][1] == 88
    assert va.LOCUS_DTYPE.itemsize == 16


def _run(*args):
    return subprocess.run([os.path.join(BIN, "guide_summary")] + list(args), capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def test_guide_summary_argument_errors(tmp_path):
    (tmp_path / "g.fa").write_text(">c\n" + "ACGT" * 30 + "\n")
    (tmp_path / "r.fa").write_text(">r\n" + "ACGT" * 5 + "AGG\n")
    (tmp_path / "t.bed").write_text("c\t0\t23\tt\t0\t+\n")
    g, r, b = str(tmp_path / "g.fa"), str(tmp_path / "r.fa"), str(tmp_path / "t.bed")
    base = ["-G", g, "-I", str(tmp_path / "idx"), "-O", str(tmp_path / "out.tsv")]
    res = _run(*base, "-R", r, "-M", "9")
    assert res.returncode == 1 and "Maximum number of mismatches must lie between 0 and 8" in res.stderr
    assert _run(*base, "-R", r, "-M", "-1").returncode == 1
    assert _run(*base, "-R", r, "-M", "x").returncode == 1
    assert _run(*base, "-R", r).returncode == 1                      # -M is required
    res = _run(*base, "-M", "3")                                     # neither -R nor -B
    assert res.returncode == 1 and "exactly one of -R" in res.stderr
    assert _run(*base, "-R", r, "-B", b, "-M", "3").returncode == 1  # both
    assert _run(*base, "-R", str(tmp_path / "r.txt"), "-M", "3").returncode == 1
    assert _run(*base, "-B", str(tmp_path / "t.txt"), "-M", "3").returncode == 1
    assert _run("-G", str(tmp_path / "g.txt"), "-I", "x", "-R", r, "-M", "3").returncode == 1
    assert _run(*base[:4], "-O", str(tmp_path / "out.sam"), "-R", r, "-M", "3").returncode == 1
    assert _run(*base, "-R", r, "-M", "3", "-D", "0,x").returncode == 1
    assert _run("--help").returncode == 0
    assert not (tmp_path / "out.tsv").exists()

"""Writes crispor_cfd.npz and cfd_table_fit.tsv from CRISPOR's output for the SITE-Seq guides of VARSCOT's pipeline comparison.

    python make_cfd_golden.py crispor-siteseq-output.txt crispor-siteseq-offtargets.txt

(both files: workflow/pipeline-comparison/ of the VARSCOT repository; the two fixtures are written beside this script).

crispor_cfd.npz - every row of the off-target file, in file order:
    guides      the guides' 23 letters ("S23"), in the order of the guide-level file
    cfd_spec    their cfdSpecScore (int)
    guide       per row: index into guides
    site        per row: offtargetSeq as a 2-bit code, base j in bits 2 j .. (A 0, C 1, G 2, T 3: vsc_pack_guide's code)
    mismatches  per row: mismatchCount
    cfd         per row: cfdOfftargetScore as printed -> float64

cfd_table_fit.tsv - the part of the CFD table these rows determine, in ScoreTable.from_tsv's format:
    fitted    a least-squares fit of log(score) over the non-zero rows: one unknown per (position, guide letter, site letter)
              and per PAM dinucleotide that occurs in them.  The system has full column rank and the fit leaves no residual
              beyond the 12 printed digits, so the weights are determined; they are rounded to nine decimals - the precision
              the published table has - if the rounded table still reproduces every non-zero row within 1e-11, else written
              with 17 significant digits.
    inferred  entries that occur in rows printed as 0.0 and in no other row: 0.
    unknown   entries no row touches: '?' (a loader has to be told what to put there).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LETTERS = "ACGT"
TOL = 1e-11


def read_rows(output_path, offtargets_path):
    guides, spec = [], []
    with open(output_path) as f:
        head = f.readline().rstrip("\n").split("\t")
        seq_col, spec_col = head.index("guideSeq"), head.index("cfdSpecScore")
        for line in f:
            row = line.rstrip("\n").split("\t")
            if len(row) > spec_col:
                guides.append(row[seq_col])
                spec.append(int(row[spec_col]))
    index = {g: i for i, g in enumerate(guides)}
    rows = []
    with open(offtargets_path) as f:
        head = f.readline().rstrip("\n").split("\t")
        cols = [head.index(c) for c in ("guideSeq", "offtargetSeq", "mismatchCount", "cfdOfftargetScore")]
        for line in f:
            row = line.rstrip("\n").split("\t")
            if len(row) > max(cols):
                g, s, mm, cfd = (row[c] for c in cols)
                assert len(s) == 23 and set(s) <= set(LETTERS), s
                rows.append((index[g], s, int(mm), float(cfd)))
    return guides, spec, rows


def entries(guide, site):
    """The table entries a (guide, site) pair multiplies: ('m', j, g, s) per mismatched position 0..19, ('p', s21, s22)."""
    e = [("m", j, LETTERS.index(guide[j]), LETTERS.index(site[j])) for j in range(20) if guide[j] != site[j]]
    return e + [("p", LETTERS.index(site[21]), LETTERS.index(site[22]))]


def product(weights, guide, site):
    x = 1.0
    for e in entries(guide, site):  # ascending position, then the PAM: the definition's order
        x = x * weights[e]
    return x


def main(output_path, offtargets_path):
    guides, spec, rows = read_rows(output_path, offtargets_path)
    positive = [r for r in rows if r[3] > 0.0]
    zero = [r for r in rows if r[3] == 0.0]
    cols = sorted({e for gi, s, _, _ in positive for e in entries(guides[gi], s)})
    col = {e: i for i, e in enumerate(cols)}
    A = np.zeros((len(positive), len(cols)))
    for i, (gi, s, _, _) in enumerate(positive):
        for e in entries(guides[gi], s):
            A[i, col[e]] += 1.0
    b = np.log([r[3] for r in positive])
    x, _, rank, _ = np.linalg.lstsq(A, b, rcond=None)
    assert rank == len(cols), (rank, len(cols))
    print("fit: %d rows, %d unknowns, rank %d, largest residual %.3g" % (len(positive), len(cols), rank, np.abs(A @ x - b).max()), file=sys.stderr)

    def worst(weights):
        return max(abs(product(weights, guides[gi], s) / cfd - 1.0) for gi, s, _, cfd in positive)

    exact = {e: float(np.exp(v)) for e, v in zip(cols, x)}
    rounded = {e: round(w, 9) for e, w in exact.items()}
    use_rounded = worst(rounded) <= TOL
    print("worst relative error: unrounded fit %.3g, nine decimals %.3g -> %s" % (worst(exact), worst(rounded),
                                                                                 "nine decimals" if use_rounded else "17 digits"), file=sys.stderr)
    weights = rounded if use_rounded else exact
    assert worst(weights) <= TOL
    inferred = sorted({e for gi, s, _, _ in zero for e in entries(guides[gi], s)} - set(cols))
    for gi, s, _, _ in zero:  # every zero row holds an entry that no non-zero row holds
        assert any(e in inferred for e in entries(guides[gi], s)), (guides[gi], s)

    def line(e, text, mark):
        if e[0] == "m":
            return "%d\t%s\t%s\t%s\t# %s" % (e[1], LETTERS[e[2]], LETTERS[e[3]], text, mark)
        return "PAM\t%s%s\t%s\t# %s" % (LETTERS[e[1]], LETTERS[e[2]], text, mark)

    every = [("m", j, g, s) for j in range(20) for g in range(4) for s in range(4) if g != s] + [("p", a, c) for a in range(4) for c in range(4)]
    out = ["# The part of the CFD table that CRISPOR's SITE-Seq off-target rows determine (make_cfd_golden.py).",
           "# j g s w: read position (0 = PAM-distal), guide letter, site letter in read orientation, weight; PAM XY w.",
           "# fitted: %d entries, %s; inferred: %d entries seen only in rows printed 0.0; unknown: %d entries no row touches."
           % (len(cols), "rounded to nine decimals" if use_rounded else "17 significant digits", len(inferred), len(every) - len(cols) - len(inferred))]
    for e in every:
        if e in weights:
            out.append(line(e, ("%.9f" if use_rounded else "%.17g") % weights[e], "fitted"))
        elif e in inferred:
            out.append(line(e, "0", "inferred"))
        else:
            out.append(line(e, "?", "unknown"))
    with open(os.path.join(HERE, "cfd_table_fit.tsv"), "w") as f:
        f.write("\n".join(out) + "\n")

    code = np.zeros(len(rows), dtype=np.uint64)
    for i, (_, s, _, _) in enumerate(rows):
        code[i] = sum(LETTERS.index(c) << (2 * j) for j, c in enumerate(s))
    np.savez_compressed(os.path.join(HERE, "crispor_cfd.npz"), guides=np.array(guides, dtype="S23"), cfd_spec=np.array(spec, dtype=np.int32),
                        guide=np.array([r[0] for r in rows], dtype=np.uint8), site=code,
                        mismatches=np.array([r[2] for r in rows], dtype=np.uint8), cfd=np.array([r[3] for r in rows], dtype=np.float64))
    print("%d rows (%d non-zero, %d zero), %d guides" % (len(rows), len(positive), len(zero), len(guides)), file=sys.stderr)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])

"""Writes crispor_guides.tsv: one row per guide of CRISPOR's guide-level output for the SITE-Seq guides of VARSCOT's
pipeline comparison - guideSeq, offtargetCount, mitSpecScore, and the sum over the guide's listed off-targets of
rint(mitOfftargetScore * 2^24) (round half to even), the fixed-point MIT sum vsc_search_summary reports.

    python make_crispor_guides.py crispor-siteseq-output.txt crispor-siteseq-offtargets.txt > crispor_guides.tsv

(both files: workflow/pipeline-comparison/ of the VARSCOT repository)."""
import sys


def main(output_path, offtargets_path):
    sums, counts = {}, {}
    with open(offtargets_path) as f:
        head = f.readline().rstrip("\n").split("\t")
        seq_col, mit_col = head.index("guideSeq"), head.index("mitOfftargetScore")
        for line in f:
            row = line.rstrip("\n").split("\t")
            if len(row) <= mit_col:
                continue
            g = row[seq_col]
            sums[g] = sums.get(g, 0) + int(round(float(row[mit_col]) * 2.0 ** 24))  # round() on a float: half to even
            counts[g] = counts.get(g, 0) + 1
    out = ["guideSeq\tofftargetCount\tmitSpecScore\tmitSumFixed24"]
    with open(output_path) as f:
        head = f.readline().rstrip("\n").split("\t")
        seq_col, spec_col, count_col = head.index("guideSeq"), head.index("mitSpecScore"), head.index("offtargetCount")
        for line in f:
            row = line.rstrip("\n").split("\t")
            if len(row) <= count_col:
                continue
            g = row[seq_col]
            assert counts.get(g, 0) == int(row[count_col]), (g, counts.get(g), row[count_col])
            out.append("%s\t%s\t%s\t%d" % (g, row[count_col], row[spec_col], sums[g]))
    sys.stdout.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])

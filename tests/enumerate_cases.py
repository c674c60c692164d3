"""Shared by tests/test_enumerate_cpu.py and tests/test_enumerate.py: the definition of a candidate guide (include/varscot_hip.h,
vsc_guides_enumerate) applied literally, window by window, in plain Python - and the edge layout, the smallest genome at which
each part of the enumeration kernels can still go wrong."""
import numpy as np

from helpers import random_seq, revcomp

WINDOW = 23
TILE = 2048
LOCUS_DTYPE = np.dtype([("contig", "<u4"), ("pos", "<u4"), ("strand", "<u4"), ("reserved", "<u4")])


def normalise(seq):
    """Upper case, everything else than ACGT is N (the packing's SeqAn Dna5 conversion)."""
    return "".join(c if c in "ACGT" else "N" for c in seq.upper())


def code_of(guide):
    """vsc_pack_guide: base i in bits 2 i, 2 i + 1, A = 0, C = 1, G = 2, T = 3."""
    return sum("ACGT".index(c) << (2 * i) for i, c in enumerate(guide))


def longest_run(s, letter):
    best = run = 0
    for c in s:
        run = run + 1 if c == letter else 0
        best = max(best, run)
    return best


def kept(guide, gc=(0, 0), max_t_run=0):
    """The sequence filters on one guide (23 letters, guide orientation): G / C and T runs of the protospacer g[0..20)."""
    proto = guide[:20]
    n_gc = proto.count("G") + proto.count("C")
    if n_gc < gc[0] or (gc[1] and n_gc > gc[1]):
        return False
    return not max_t_run or longest_run(proto, "T") <= max_t_run


def brute_force(contigs, pam="GG", strands="both", gc=(0, 0), max_t_run=0, member=None):
    """[(contig, pos, strand, guide)] in the order of the result: ascending (contig, pos), '+' before '-'.
    member: None, or per contig a bool array over its positions - is the window that starts there in the regions
    (regions_cases.brute_force(intervals, lens)[rule])."""
    pam = pam.upper()
    rc_pam = revcomp(pam)
    out = []
    for c, raw in enumerate(contigs):
        s = normalise(raw)
        for p in range(len(s) - WINDOW + 1):
            w = s[p:p + WINDOW]
            if "N" in w or (member is not None and not member[c][p]):
                continue
            if strands in ("both", "+") and w[21:23] == pam and kept(w, gc, max_t_run):
                out.append((c, p, 0, w))
            if strands in ("both", "-") and w[0:2] == rc_pam:
                g = revcomp(w)
                if kept(g, gc, max_t_run):
                    out.append((c, p, 1, g))
    return out


def arrays(cands):
    """(codes uint64[n], loci LOCUS_DTYPE[n]) of a brute_force list: what Genome.enumerate_guides returns."""
    codes = np.array([code_of(g) for _, _, _, g in cands], dtype=np.uint64)
    loci = np.zeros(len(cands), dtype=LOCUS_DTYPE)
    if cands:
        loci["contig"], loci["pos"], loci["strand"] = (np.array([x[k] for x in cands], dtype=np.uint32) for k in range(3))
    return codes, loci


def global_positions(contigs, cands):
    """Global position of every candidate's window start: contigs are laid out with one separator position between them."""
    off = np.concatenate([[0], np.cumsum([len(s) + 1 for s in contigs])])
    return np.array([off[c] + p for c, p, _, _ in cands], dtype=np.int64)


# guides for the T-run cases of the random contig (guide orientation, NGG):
T_INSIDE = "ACGATTTTCAGCATGCAGACAGG"   # TTTT in the protospacer: dropped by max_t_run = 3
T_AT_PAM = "ACGATCGACAGCATGCATTTTGG"   # g[17..21) = TTTT: three T in the protospacer, the fourth is the N of NGG - kept
RANDOM_AT = 5  # index of the random contig in the edge layout
PLANTS = [(2000, T_INSIDE, "+"), (2100, T_INSIDE, "-"), (2200, T_AT_PAM, "+"), (2300, T_AT_PAM, "-")]


def edge_layout():
    """The contigs of the edge layout, in order:
    full masks over more than two tiles on '+' and on '-', a 23-base contig with both strands at position 0 (p + 23 == L),
    contigs without candidates (too short; an N in the middle), a random contig with an N run, lower case, an IUPAC letter and
    the planted T runs, and G-only as the last contig."""
    rng = np.random.default_rng(4711)
    r = list(random_seq(rng, 14000))
    for pos, guide, strand in PLANTS:
        r[pos:pos + WINDOW] = guide if strand == "+" else revcomp(guide)
    r[5000:5050] = "N" * 50
    r[7000:7300] = "".join(r[7000:7300]).lower()
    r[9000] = "R"
    return ["G" * 4200, "C" * 4200, "CC" + "A" * 19 + "GG", "G" * 22, "G" * 11 + "N" + "G" * 12, "".join(r), "G" * 40]


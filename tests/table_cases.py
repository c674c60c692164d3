"""Shared helpers of test_table.py (GPU) and test_table_cpu.py: the definition of the table score in plain Python, the CRISPOR
fixture (tests/golden/crispor_cfd.npz, cfd_table_fit.tsv), random tables, and the numpy aggregation and cut the table sinks are
checked against over the record route (search + the host's scores)."""
import os

import numpy as np

import varscot_amd as va
from helpers import cut, revcomp
from varscot_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABLE_TSV = os.path.join(GOLDEN, "cfd_table_fit.tsv")
ONE = 1 << 30
CFD_SPEC = [46, 50, 35, 68, 50, 67, 62]  # cfdSpecScore of the seven SITE-Seq guides (crispor-siteseq-output.txt)
REL_TOL = 1e-11  # CRISPOR prints 12 significant digits (<= 5e-12 relative) + a few ulps of product order


def code(letter):
    """vsc_pack_guide's code of a letter: non-ACGT becomes A."""
    return max("ACGT".find(letter.upper()), 0)


def py_score(pair, pam, guide, site):
    """The definition (include/varscot_hip.h, SCORE) over nested lists / arrays of Python floats: IEEE doubles, fixed order."""
    x = 1.0
    for j in range(20):
        g, s = code(guide[j]), code(site[j])
        if g != s:
            x = x * float(pair[j][g][s])
    return x * float(pam[4 * code(site[21]) + code(site[22])])


def py_fixed(x):
    return int(np.rint(x * 2.0 ** 30))  # np.rint: round half to even


def fixture_table():
    """The fitted part of the CFD table; the entries no fixture row touches are filled with 0.5."""
    return va.ScoreTable.from_tsv(TABLE_TSV, default=0.5)


def fixture_rows():
    """crispor_cfd.npz as a dict: guides (list of str), cfd_spec, and per row guide, site (str), mismatches, cfd."""
    z = np.load(os.path.join(GOLDEN, "crispor_cfd.npz"))
    return dict(guides=[g.decode() for g in z["guides"]], cfd_spec=z["cfd_spec"].tolist(), guide=z["guide"].astype(np.int64),
                site_code=z["site"], site=va.unpack_guides(z["site"]), mismatches=z["mismatches"].astype(np.int64), cfd=z["cfd"])


def random_table(rng, zeros=0, ones=0):
    """(pair, pam) with weights in (0, 1), the diagonal 1, and that many off-diagonal entries set to exactly 0 / 1."""
    pair = rng.uniform(0.01, 0.99, size=(20, 4, 4))
    pam = rng.uniform(0.01, 0.99, size=16)
    off = [(j, g, s) for j in range(20) for g in range(4) for s in range(4) if g != s]
    pick = rng.permutation(len(off))
    for k in pick[:zeros]:
        pair[off[k]] = 0.0
    for k in pick[zeros:zeros + ones]:
        pair[off[k]] = 1.0
    for b in range(4):
        pair[:, b, b] = 1.0
    return pair, pam


def site_text(contigs, h):
    """A hit's 23-base window in read orientation."""
    w = contigs[int(h["contig"])][int(h["pos"]):int(h["pos"]) + 23]
    return revcomp(w) if int(h["info"]) >> 31 else w


def host_scores(table, guides, contigs, hits):
    """(score float64, fixed int64) per record, by vsc_table_score over the guide and the site's text in read orientation."""
    x, f = np.zeros(len(hits)), np.zeros(len(hits), dtype=np.int64)
    for i, h in enumerate(hits):
        x[i], f[i] = table.score(guides[int(h["guide"])], site_text(contigs, h), fixed=True)
    return x, f


def numpy_scores(table, guides, contigs, hits):
    """host_scores for many records: the definition's loop over the 20 positions, vectorised over the records - the same IEEE
    multiplications in the same order, so the same bits (test_table.py checks that once per genome against host_scores)."""
    lut = np.zeros(256, dtype=np.int64)
    for i, c in enumerate("ACGT"):
        lut[ord(c)] = lut[ord(c.lower())] = i
    g = lut[np.frombuffer("".join(guides).encode(), dtype=np.uint8).reshape(len(guides), 23)][hits["guide"].astype(np.int64)]
    s = lut[np.frombuffer("".join(site_text(contigs, h) for h in hits).encode(), dtype=np.uint8).reshape(len(hits), 23)]
    x = np.ones(len(hits))
    for j in range(20):
        x = np.where(g[:, j] != s[:, j], x * table.pair[j, g[:, j], s[:, j]], x)
    x = x * table.pam[4 * s[:, 21] + s[:, 22]]
    return x, np.rint(x * 2.0 ** 30).astype(np.int64)


def counted(hits, exclude):
    keep = np.ones(len(hits), dtype=bool)
    if exclude is not None:
        ex = np.array(exclude, dtype=np.int64).reshape(-1, 3)
        g = hits["guide"].astype(np.int64)
        keep = ~((ex[g, 0] == hits["contig"]) & (ex[g, 1] == hits["pos"]) & (ex[g, 2] == (hits["info"] >> 31)))
    return keep


def table_rows(guide, nm, fixed, n_guides):
    """The vsc_guide_table_row rows of a table of counted hits (guide index, NM, fixed-point score per hit): plain sums."""
    guide, nm, fixed = (np.asarray(a, dtype=np.int64) for a in (guide, nm, fixed))
    rows = np.zeros(n_guides, dtype=_lib.TABLE_ROW_DTYPE)
    np.add.at(rows["score_sum"], guide, fixed.astype(np.uint64))
    pos = fixed > 0
    rows["positive"] = np.bincount(guide[pos], minlength=n_guides)
    for k in range(9):
        rows["positive_nm"][:, k] = np.bincount(guide[pos & (nm == k)], minlength=n_guides)
    return rows


def rows_of_hits(hits, fixed, n_guides, exclude=None):
    keep = counted(hits, exclude)
    return table_rows(hits["guide"][keep], (hits["info"][keep] >> 23) & 31, np.asarray(fixed)[keep], n_guides)


def cut_by_table(hits, fixed, top_k=0, min_score=0, exclude=None, ranked=False):
    """The selection by table score on the host: helpers.cut with the fixed-point scores as the key."""
    return cut(hits, fixed, top_k=top_k, min_score=min_score, exclude=exclude, ranked=ranked)


def record_route(gen, table, guides, contigs, m, algorithm, extra_pam=None):
    """(records, scores, fixed) the way the library offered them before the table sinks: every record materialised, scored on the host."""
    h = gen.search(guides, m, algorithm=algorithm, extra_pam=extra_pam)
    rec = h.to_numpy().copy()
    h.close()
    x, f = numpy_scores(table, guides, contigs, rec)
    return rec, x, f


def selected(gen, guides, m, table, **kw):
    h = gen.search_select_table(guides, m, table, **kw)
    if isinstance(h, tuple):
        got = (h[0].to_numpy().copy(),) + h[1:]
        h[0].close()
        return got
    got = h.to_numpy().copy()
    h.close()
    return got

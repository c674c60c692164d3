"""The bulge search's definition (include/varscot_hip.h, vsc_search_bulges) restated in plain Python, and the scenarios the
tests run it on.  Nothing here calls the library: best() is the definition for one read and one site, brute_force() applies it
site by site (numpy over the sites of one class where the plain loop is slow), and every scenario asserts floors on the
restatement's OWN output, so that no branch of the definition is empty in it."""
import numpy as np

READ_LEN = 23
TILE = 2048
CLASSES = (-2, -1, 1, 2)  # ascending d: the row order of vsc_bulge_summary
COMP = str.maketrans("ACGTN", "TGCAN")
HIT_DTYPE = np.dtype([("guide", "<u4"), ("contig", "<u4"), ("pos", "<u4"), ("info", "<u4")])


def rc(s):
    return s.translate(COMP)[::-1]


def read_of(text):
    """A read as the searches take it: upper case, non-ACGT becomes A."""
    return "".join(ch if ch in "ACGT" else "A" for ch in text.upper())


def genome_of(text):
    """Genome letters: ACGT in any case are bases, everything else is N."""
    return "".join(ch if ch in "ACGT" else "N" for ch in text.upper())


def max_index(d):
    return 19 if d > 0 else 19 + d


def nm_at(r, s, d, i):
    """nm(i) of the definition: r a 23-letter read, s a site of 23 + d letters in read orientation."""
    if d > 0:
        return sum(r[j] != s[j] for j in range(i)) + sum(r[j] != s[j + d] for j in range(i, READ_LEN))
    b = -d
    return sum(r[j] != s[j] for j in range(i)) + sum(r[j] != s[j - b] for j in range(i + b, READ_LEN))


def best(r, s, d):
    """(NM, index, tie): the minimum of nm(i), the smallest i that reaches it, and whether a larger i reaches it too."""
    assert len(r) == READ_LEN and len(s) == READ_LEN + d and d in CLASSES
    all_nm = [nm_at(r, s, d, i) for i in range(1, max_index(d) + 1)]
    nm = min(all_nm)
    return nm, 1 + all_nm.index(nm), all_nm.count(nm) > 1


def enabled(dna, rna):
    return [d for d in CLASSES if (d > 0 and d <= dna) or (d < 0 and -d <= rna)]


def candidates(contigs, dna, rna, extra_pam=None):
    """Every (strand, contig, pos, d, s): conditions 1 to 3 of the definition, s in read orientation."""
    pams = {"GG", "GA"} | ({extra_pam.upper()} if extra_pam else set())
    out = []
    for c, raw in enumerate(contigs):
        seq = genome_of(raw)
        for p in range(len(seq)):
            for d in enabled(dna, rna):
                L = READ_LEN + d
                if p + L > len(seq):
                    continue
                w = seq[p:p + L]
                if "N" in w:
                    continue
                for strand in (0, 1):
                    s = w if strand == 0 else rc(w)
                    if s[L - 2:] in pams:
                        out.append((strand, c, p, d, s))
    return out


def _codes(text):
    return np.frombuffer(text.encode(), dtype=np.uint8)


def brute_force(contigs, guides, m, dna, rna, extra_pam=None, cands=None):
    """The hits as (guide, strand, contig, pos, d, nm, index, tie) in ascending (guide, strand, contig, pos, d) order.
    Condition 4 is evaluated for all sites of one class at a time: nm(i) exactly as nm_at writes it, with numpy sums."""
    cands = candidates(contigs, dna, rna, extra_pam) if cands is None else cands
    hits = []
    for d in enabled(dna, rna):
        sub = [x for x in cands if x[3] == d]
        if not sub:
            continue
        S = np.stack([_codes(x[4]) for x in sub])  # [n, 23 + d]
        for g, text in enumerate(guides):
            r = _codes(read_of(text))
            rows = []
            for i in range(1, max_index(d) + 1):
                if d > 0:
                    nm = (S[:, :i] != r[:i]).sum(1) + (S[:, i + d:READ_LEN + d] != r[i:]).sum(1)
                else:
                    b = -d
                    nm = (S[:, :i] != r[:i]).sum(1) + (S[:, i:READ_LEN - b] != r[i + b:]).sum(1)
                rows.append(nm)
            A = np.stack(rows)  # [index - 1, site]
            nm_min = A.min(0)
            first = A.argmin(0) + 1
            ties = (A == nm_min).sum(0) > 1
            for k in np.nonzero(nm_min <= m)[0]:
                strand, c, p, _, _ = sub[k]
                hits.append((g, strand, c, p, d, int(nm_min[k]), int(first[k]), bool(ties[k])))
    hits.sort(key=lambda h: h[:5])
    return hits


def info_word(strand, d, index, nm):
    return strand << 31 | (1 if d < 0 else 0) << 12 | abs(d) << 10 | index << 5 | nm


def arrays(hits, n_guides):
    """(records, rows) as vsc_search_bulges returns them."""
    rec = np.zeros(len(hits), dtype=HIT_DTYPE)
    rows = np.zeros((n_guides, 4, 9), dtype=np.uint32)
    for k, (g, strand, c, p, d, nm, index, _) in enumerate(hits):
        rec[k] = (g, c, p, info_word(strand, d, index, nm))
        rows[g, CLASSES.index(d), nm] += 1
    return rec, rows


def d_of_info(info):
    info = np.asarray(info, dtype=np.uint32)
    size = ((info >> 10) & 3).astype(np.int64)
    return np.where((info >> 12) & 1 == 1, -size, size)


def merge_order(rec):
    """The indices that put records into ascending (guide, strand, contig, pos, d) order."""
    return np.lexsort((d_of_info(rec["info"]), rec["pos"], rec["contig"], rec["info"] >> 31, rec["guide"]))


# ---- scenarios ------------------------------------------------------------------------------------------------------------
def rnd(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(0, 4, n))


def plant(rng, read, d, i, subs=(), bulge=None):
    """A site of 23 + d letters in read orientation that pairs with `read` at split point i with the substitutions `subs`
    (read positions outside the bulge): a DNA bulge inserts `bulge` (default: letters that differ from both neighbours, so that
    no smaller i pairs as well), an RNA bulge drops read[i .. i - d)."""
    r = list(read)
    for j in subs:
        r[j] = "ACGT"[("ACGT".index(r[j]) + 1 + int(rng.integers(0, 3))) % 4]
    r = "".join(r)
    if d > 0:
        if bulge is None:
            bulge = ""
            for _ in range(d):
                bulge += next(x for x in "ACGT" if x not in (read[i - 1], read[i], bulge[-1:] or "-"))
        assert len(bulge) == d
        return r[:i] + bulge + r[i:]
    return r[:i] + r[i - d:]


def distinct_read(rng, pam="TGG"):
    """A read whose protospacer has no equal letters at distance 1 or 2: a planted bulge then has one best split point."""
    p = []
    for j in range(20):
        p.append(next(str(x) for x in rng.permutation(list("ACGT")) if x not in p[-2:]))
    return "".join(p) + pam


def put(seq, pos, site):
    return seq[:pos] + site + seq[pos + len(site):]


EDGE_M = 4


def edge_scenario():
    """Contigs, guides and the restatement's hits at m = 4, dna = rna = 2 - with the edge cases of the search's front end and
    floors on the hits (asserted here)."""
    rng = np.random.default_rng(20260)
    g0, g1, g2 = distinct_read(rng), distinct_read(rng, "AGG"), distinct_read(rng, "CGA")
    # both strands at one start: w pairs with g3 on '+' (DNA 1 at index 7) and its reverse complement with g4 on '-' (DNA 1 at 12)
    g3 = "CC" + rnd(rng, 18) + "AGG"
    both = g3[:7] + ("T" if g3[6] != "T" and g3[7] != "T" else "A") + g3[7:]
    g4 = rc(both)[:12] + rc(both)[13:]
    g5 = rnd(rng, 9) + "N" + rnd(rng, 10) + "TGG"  # a read with a non-ACGT letter: it is searched as A
    g6 = rnd(rng, 20) + "GGA"
    guides = [g0, g1, g2, g3, g4, g5, g6]
    reads = [read_of(g) for g in guides]

    big = rnd(rng, 5200)
    planted = []  # (strand, site on the forward genome): every class, strand, index 1 / largest / another, 0 .. m substitutions
    k = 0
    for d in CLASSES:
        for strand in (0, 1):
            for i in (1, max_index(d), 2 + (k % (max_index(d) - 2))):
                for n_subs in range(EDGE_M + 1):
                    read = reads[k % 3]  # the reads without ties
                    free = [j for j in range(21) if j < i - 1 or j > i + 2]  # (not the PAM, not beside or in the bulge)
                    site = plant(rng, read, d, i, rng.choice(free, size=n_subs, replace=False))
                    planted.append((strand, site if strand == 0 else rc(site)))
                    k += 1
    order = [int(x) for x in rng.permutation(len(planted))]
    take = lambda strand: planted[order.pop(next(n for n, x in enumerate(order) if planted[x][0] == strand))][1]
    # p = 0; across the first tile end on '+' and the second on '-'; then one site every 97 bases (most cross a 32-base word)
    body = put(big, 0, take(0))
    body = put(body, TILE - 10, take(0))
    body = put(body, 2 * TILE - 13, take(1))
    for pos in [100 + 97 * n for n in range(41) if not any(abs(100 + 97 * n - q) < 60 for q in (TILE, 2 * TILE))]:
        body = put(body, pos, planted[order.pop()][1])
    free_at = 4200
    # the sites that found no place there: one behind the other with random spacers, in a contig of their own
    tail = "".join(rnd(rng, int(rng.integers(3, 40))) + planted[x][1] for x in order)
    body = put(body, free_at, both)
    # a tie: the inserted base repeats its left neighbour, so index i - 1 and i pair alike and the smaller is reported
    tie_site = reads[0][:9] + reads[0][8] + reads[0][9:]
    body = put(body, 4300, tie_site)
    # an N at the bulged base and an IUPAC letter inside a site: absent; a lower-case site: present
    body = put(body, 4400, reads[1][:6] + "N" + reads[1][6:])
    body = put(body, 4500, (reads[1][:6] + "T" + reads[1][6:])[:14] + "R" + (reads[1][:6] + "T" + reads[1][6:])[15:])
    body = put(body, 4600, plant(rng, reads[2], 1, 5).lower())
    body = put(body, 4700, rc(plant(rng, reads[2], -1, 5)).lower())
    # p + L == len(c): the contig ends with a site
    body = body[:5200 - 25] + plant(rng, reads[0], 2, 10)
    # a site that would span two contigs: its first 12 bases end one contig, the rest starts the next
    span = plant(rng, reads[1], 1, 8)
    left, right = rnd(rng, 150) + span[:12], span[12:] + rnd(rng, 150)
    # contigs shorter than 25 and of exactly 21 to 25 bases: each a site of its own length where one exists
    small = [rnd(rng, 20), plant(rng, reads[0], -2, 4), rc(plant(rng, reads[1], -1, 9)), reads[2], plant(rng, reads[0], 1, 3),
             rc(plant(rng, reads[2], 2, 15)), rnd(rng, 7)]
    assert [len(s) for s in small] == [20, 21, 22, 23, 24, 25, 7]
    contigs = [body, left, right] + small + [tail, rnd(rng, 300)]
    total = sum(len(c) for c in contigs)
    assert 6000 <= total <= 10500, total

    cands = candidates(contigs, 2, 2)
    hits = brute_force(contigs, guides, EDGE_M, 2, 2, cands=cands)
    # ---- floors ----
    for d in CLASSES:
        for strand in (0, 1):
            mine = [h for h in hits if h[4] == d and h[1] == strand]
            assert {h[5] for h in mine} == set(range(EDGE_M + 1)), (d, strand)       # every class, strand and NM
            assert {1, max_index(d)} <= {h[6] for h in mine}, (d, strand)            # index 1 and the largest legal one
    assert any(h[7] and h[6] == 8 and h[4] == 1 and h[2] == 0 and h[3] == 4300 for h in hits)  # the tie, resolved downwards
    starts = {(h[1], h[2], h[3]) for h in hits}
    assert (0, 0, 0) in starts or (1, 0, 0) in starts                                # p = 0
    assert any(h[2] == 0 and h[3] + READ_LEN + h[4] == len(body) for h in hits)      # p + L == len(c)
    for s in (0, 1):
        assert any(h[1] == s and h[2] == 0 and h[3] < (1 + s) * TILE < h[3] + READ_LEN + h[4] for h in hits), s  # across a tile end
        assert any(h[1] == s and h[2] == 0 and h[3] // 32 != (h[3] + READ_LEN + h[4] - 1) // 32 for h in hits), s
    assert (0, 0, free_at) in starts and (1, 0, free_at) in starts                   # both strands at one start
    assert not any(h[2] == 0 and h[3] in (4400, 4500) and h[5] <= 1 for h in hits)   # N / IUPAC at or in the site
    assert any(h[2] == 0 and h[3] == 4600 and h[0] == 2 for h in hits)               # lower case
    assert any(h[2] == 0 and h[3] == 4700 and h[0] == 2 and h[1] == 1 for h in hits)
    assert not any(h[2] in (1, 2) and h[0] == 1 and h[5] == 0 for h in hits)         # the site across two contigs
    for c, d in ((4, -2), (5, -1), (7, 1), (8, 2)):                                 # contigs that are one site
        assert any(h[2] == c and h[3] == 0 and h[4] == d and h[5] == 0 for h in hits), c
    assert not any(h[2] in (3, 9) for h in hits)                                     # contigs too short for any site
    return {"contigs": contigs, "guides": guides, "cands": cands, "hits": hits}


def tandem_scenario():
    """One 24-base site (a DNA bulge of 1 for the read), 210 copies back to back across two tile ends."""
    rng = np.random.default_rng(20261)
    read = distinct_read(rng)
    site = plant(rng, read, 1, 11)
    contigs = [rnd(rng, 1000) + site * 210 + rnd(rng, 400)]
    guides = [read, distinct_read(rng, "AGG")]
    hits = brute_force(contigs, guides, 3, 1, 1)
    copies = [h for h in hits if h[0] == 0 and h[1] == 0 and h[4] == 1 and h[5] == 0]
    assert len(copies) >= 200
    assert min(h[3] for h in copies) < TILE < 2 * TILE < max(h[3] for h in copies)
    assert max(np.bincount([h[3] // 32 for h in hits if h[0] == 0])) >= 2  # more than one hit in a lane's 32 starts
    return {"contigs": contigs, "guides": guides, "hits": hits}

"""Pattern guide discovery (include/varscot_hip.h, vsc_guides_enumerate_pattern) restated in plain Python, site by site, and the
scenarios the tests run it on.  Nothing here calls the library.  candidates() applies conditions 1-3 to every start and both
strands, kept() the filters and the target rule to every candidate, arrays() packs what is left as the call returns it; every
scenario asserts floors on the restatement's OWN output, so that no edge it is built for is missing from it."""
import functools

import numpy as np

import pattern_cases as pc

TILE = pc.TILE
LOCUS_DTYPE = np.dtype([("contig", "<u4"), ("pos", "<u4"), ("strand", "<u4"), ("reserved", "<u4")])


# ---- the definition -------------------------------------------------------------------------------------------------------
def candidates(contigs, pattern):
    """Every CANDIDATE as (contig, pos, strand, s), s = the site in read orientation, in ascending (contig, pos), '+' first."""
    L = len(pattern)
    sets = [pc.IUPAC[ch] for ch in pattern.upper()]
    out = []
    for c, raw in enumerate(contigs):
        seq = pc.genome_of(raw)
        for p in range(len(seq) - L + 1):             # p + L <= len(c)
            w = seq[p:p + L]
            if "N" in w:                              # a non-ACGT genome letter
                continue
            for strand in (0, 1):
                s = w if strand == 0 else pc.rc(w)
                if all(s[j] in sets[j] for j in range(L)):
                    out.append((c, p, strand, s))
    return out


def longest_t_run(text):
    best = run = 0
    for ch in text:
        run = run + 1 if ch == "T" else 0
        best = max(best, run)
    return best


def in_targets(c, p, L, targets, rule, lens):
    """The rule applied to the L-base site that starts at (c, p): end clipped to the contig, empty intervals dropped."""
    for tc, start, end in targets:
        end = min(end, lens[tc])
        if tc != c or start >= end:
            continue
        if rule == "overlap" and p < end and p + L > start:
            return True
        if rule == "inside" and start <= p and p + L <= end:
            return True
    return False


def kept(cands, contigs, L, protospacer, strands=0, gc=(0, 0), max_t_run=0, targets=None, rule="overlap"):
    """The candidates that are KEPT, filter by filter."""
    a, k = protospacer
    lens = [len(x) for x in contigs]
    out = []
    for c, p, strand, s in cands:
        if strands == 1 and strand != 0 or strands == 2 and strand != 1:
            continue
        proto = s[a:a + k]
        n_gc = sum(ch in "GC" for ch in proto)
        if n_gc < gc[0] or (gc[1] and n_gc > gc[1]):
            continue
        if max_t_run and longest_t_run(proto) > max_t_run:
            continue
        if targets is not None and not in_targets(c, p, L, targets, rule, lens):
            continue
        out.append((c, p, strand, s))
    return out


def code_of(s):
    """hi plane << 32 | lo plane, bit j = s[j], A 00 C 01 G 10 T 11."""
    hi = sum(("ACGT".index(ch) >> 1) << j for j, ch in enumerate(s))
    lo = sum(("ACGT".index(ch) & 1) << j for j, ch in enumerate(s))
    return hi << 32 | lo


def arrays(found):
    """(codes, loci) as the call returns them."""
    codes = np.array([code_of(s) for _, _, _, s in found], dtype=np.uint64)
    loci = np.zeros(len(found), dtype=LOCUS_DTYPE)
    for i, (c, p, strand, _) in enumerate(found):
        loci[i] = (c, p, strand, 0)
    return codes, loci


def guide_text(s, protospacer, spell):
    """vsc_pattern_guide_text, letter by letter."""
    a, k = protospacer
    return "".join(ch if (a <= j < a + k or spell) else "N" for j, ch in enumerate(s))


def start_ranges(contig_lens, targets, rule, L):
    """The starts that qualify, per site by brute force: the set of (contig, pos) over EVERY position of every contig (the
    sites that leave the contig included: the normalisation clips to the contig, the candidates to p + L <= len)."""
    return {(c, p) for c, n in enumerate(contig_lens) for p in range(n) if in_targets(c, p, L, targets, rule, contig_lens)}


# ---- scenarios ------------------------------------------------------------------------------------------------------------
def n_run(pattern):
    """The protospacer of a pattern_cases pattern: its run of N."""
    first = pattern.index("N")
    return first, len(pattern[first:]) - len(pattern[first:].lstrip("N"))


@functools.lru_cache(maxsize=None)
def edge_scenario(L, place):
    """pattern_cases.edge_scenario's contigs and pattern, the protospacer = the pattern's N run, no filter."""
    e = pc.edge_scenario(L, place)
    contigs, pattern = e["contigs"], e["pattern"]
    proto = n_run(pattern)
    assert pattern[proto[0]:proto[0] + proto[1]] == "N" * proto[1] and proto[1] == L - (4 if place == "both" else 3)
    cands = candidates(contigs, pattern)
    assert len(cands) == e["n_cands"]                                                   # the search's own count of candidates
    body = len(contigs[0])
    on = lambda c, p, strand: any(x[:3] == (c, p, strand) for x in cands)
    assert {x[2] for x in cands} == {0, 1}                                              # both strands
    assert any(x[0] == 0 and x[1] == 0 for x in cands)                                  # p = 0
    assert on(0, body - L, 0)                                                           # p + L == len(c)
    assert 5727 % 32 == 31 and on(0, 5727, 0)                                           # bit 31 of a word
    for strand in (0, 1):                                                               # across a tile end, either strand
        assert any(x[0] == 0 and x[2] == strand and x[1] < t < x[1] + L for x in cands for t in (TILE, 2 * TILE)), strand
    assert len(contigs[3]) == L - 1 and not any(x[0] == 3 for x in cands)               # the contig of L - 1 bases
    assert not any(x[0] == 0 and x[1] <= q < x[1] + L for x in cands for q in (5200 + L // 2, 5300 + L // 2))  # over N / IUPAC
    assert all(x[1] + L <= len(contigs[x[0]]) for x in cands)                           # none across two contigs
    assert on(0, 5600, 0)
    if place == "both":
        both = [x for x in cands if x[:2] == (0, 5600)]
        assert [x[2] for x in both] == [0, 1]                                           # two candidates at one start, '+' first
    return {"L": L, "pattern": pattern, "protospacer": proto, "contigs": contigs, "cands": cands}


@functools.lru_cache(maxsize=None)
def full_scenario():
    """N x 16: every N-free start is a candidate on both strands - full lanes, the rank arithmetic."""
    rng = np.random.default_rng(16016)
    contigs = [pc.rnd(rng, 2 * TILE + 37), pc.rnd(rng, 15), pc.rnd(rng, 16), pc.rnd(rng, 17)]
    cands = candidates(contigs, "N" * 16)
    assert len(cands) == sum(2 * (len(c) - 15) for c in contigs if len(c) >= 16) == 2 * (2 * TILE + 22) + 2 + 4
    return {"L": 16, "pattern": "N" * 16, "protospacer": (0, 16), "contigs": contigs, "cands": cands}


SA_PATTERN = "N" * 21 + "NNGRRT"      # SaCas9: protospacer (0, 21)
FIVE_PATTERN = "TTN" + "N" * 17       # a PAM at the 5' end, L = 20: protospacer (3, 17)
FILTERS = (dict(gc=(12, 0)), dict(gc=(0, 9)), dict(gc=(9, 12)), dict(max_t_run=1), dict(max_t_run=3), dict(strands=1), dict(strands=2))


def _no_t_run(rng, n, longest):
    """n random letters without a run of more than `longest` T, that neither begin nor end with T."""
    while True:
        s = pc.rnd(rng, n)
        if longest_t_run(s) <= longest and s[0] != "T" and s[-1] != "T":
            return s


@functools.lru_cache(maxsize=None)
def filter_scenario(which):
    """A random genome of two tiles and a half with planted sites, both strands each:
    "sa":   under N x 21 + NNGRRT, protospacer (0, 21): TTT at read positions 18..20 followed by a T at 21 - a run of 3, not 4
    "five": under TTN + N x 17, protospacer (3, 17): TTT at 3..5 behind the T at 2 - a run of 3, not 4
    and a TTTT inside the protospacer, which max_t_run = 3 drops."""
    rng = np.random.default_rng({"sa": 2127, "five": 2120}[which])
    pattern, proto = (SA_PATTERN, (0, 21)) if which == "sa" else (FIVE_PATTERN, (3, 17))
    L = len(pattern)
    if which == "sa":
        edge_site = _no_t_run(rng, 18, 2) + "TTT" + "T" + "AGAAT"        # s[18..21) = TTT, s[21] = T of the PAM
        inner = _no_t_run(rng, 8, 2) + "TTTT" + _no_t_run(rng, 9, 2) + "AAGAAT"
    else:
        edge_site = "TT" + "T" + "TTT" + _no_t_run(rng, 14, 2)           # s[2] = T of the PAM's N, s[3..6) = TTT
        inner = "TTA" + _no_t_run(rng, 6, 2) + "TTTT" + _no_t_run(rng, 7, 2)
    assert len(edge_site) == L and len(inner) == L
    body = pc.rnd(rng, 2 * TILE + 1000)
    where = {}
    for k, (name, site) in enumerate((("edge", edge_site), ("inner", inner))):
        for strand in (0, 1):
            pos = 700 + 1900 * k + 611 * strand
            body = pc.put(body, pos, site if strand == 0 else pc.rc(site))
            where[(name, strand)] = pos
    contigs = [body, pc.rnd(rng, 90)]
    cands = candidates(contigs, pattern)
    e = {"L": L, "pattern": pattern, "protospacer": proto, "contigs": contigs, "cands": cands, "where": where}
    # ---- floors ----
    for f in FILTERS:
        left = kept(cands, contigs, L, proto, **f)
        for strand in (0, 1):
            if f.get("strands") in (None, strand + 1):
                assert any(x[2] == strand for x in left), (f, strand)                    # keeps one ...
            if f.get("strands") != strand + 1:
                assert sum(x[2] == strand for x in left) < sum(x[2] == strand for x in cands), (f, strand)  # ... and drops one
    at3 = {x[:3] for x in kept(cands, contigs, L, proto, max_t_run=3)}
    at2 = {x[:3] for x in kept(cands, contigs, L, proto, max_t_run=2)}
    for strand in (0, 1):
        spot = (0, where[("edge", strand)], strand)
        assert spot in at3 and spot not in at2, spot                                     # a run of 3: the PAM's T does not extend it
        assert (0, where[("inner", strand)], strand) not in at3
        assert (0, where[("inner", strand)], strand) in {x[:3] for x in cands}
    return e


# The interval shapes of the target tests, on a first contig of `n` bases and a small second one (CPU: the normalisation;
# GPU: the call).  L is the site length they are meant for (20).
TARGET_L = 20


def target_intervals(n, small):
    return [
        (0, 1500, 1600), (0, 1550, 1700),             # overlapping
        (0, 500, 900), (0, 600, 700),                 # nested
        (0, 1000, 1100), (0, 1100, 1200),             # abutting: a site across the seam is inside neither
        (0, 1800, 1810),                              # shorter than L: overlap keeps sites, inside none
        (0, 5, 40),                                   # start < L - 1: the range of starts is cut at 0
        (0, n - 30, n + 1000),                        # the end past the contig: clipped
        (0, 300, 300), (0, n + 5, n + 9),             # empty, and empty after clipping
        (0, TILE - 12, TILE + 12),                    # across a tile boundary
        (0, 2 * TILE + 31, 2 * TILE + 33),            # two bases around a word boundary
        (1, 10, small - 5),                           # on the small contig
        (1, small - 2, small + 7),
    ]


TARGET_PATTERN = "N" * 19 + "R"                       # dense: half of all sites on either strand


@functools.lru_cache(maxsize=None)
def target_scenario():
    """A contig of three tiles and 300 bases and a small one, a dense pattern of L = 20 and the interval shapes above."""
    rng = np.random.default_rng(2020)
    n, small = 3 * TILE + 300, 61
    contigs = [pc.rnd(rng, n), pc.rnd(rng, small)]
    targets = target_intervals(n, small)
    L = TARGET_L
    cands = candidates(contigs, TARGET_PATTERN)
    e = {"L": L, "pattern": TARGET_PATTERN, "protospacer": (0, 19), "contigs": contigs, "cands": cands, "targets": targets,
         "last_tile": [(0, 3 * TILE + 100, 3 * TILE + 150)]}
    over = {x[:3] for x in kept(cands, contigs, L, (0, 19), targets=targets, rule="overlap")}
    ins = {x[:3] for x in kept(cands, contigs, L, (0, 19), targets=targets, rule="inside")}
    assert ins < over and len(ins) >= 100
    assert any(p < 1100 < p + L for _, p, _ in over) and not any(p < 1100 < p + L for c, p, _ in ins if c == 0)  # the seam
    assert any(1800 - L < p < 1810 for c, p, _ in over if c == 0) and not any(1790 <= p < 1810 for c, p, _ in ins if c == 0)
    assert any(p < 5 for c, p, _ in over if c == 0) and any(p + L > n - 30 for c, p, _ in over if c == 0)
    assert any(p < TILE < p + L for c, p, _ in ins if c == 0)                           # inside the interval across the tile end
    assert any(c == 1 for c, _, _ in ins) and any(c == 1 and p + L > small - 2 for c, p, _ in over)
    assert {s for _, _, s in ins} == {0, 1}
    return e

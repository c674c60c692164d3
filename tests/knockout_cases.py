"""Shared helpers of test_knockout.py (GPU) and test_knockout_cpu.py: the definition of knock-out design (include/varscot_hip.h:
SHAPE, CUT, DEFINED, CODING CUT, TRANSCRIPT, K, SHIFTED, WALK, NMD, ROW, COVERAGE, FILTER) in plain Python on strings, and the
small genome of the tests.  A different formulation from the library's cursor: every transcript's coding text T is sliced and
reverse-complemented out of its contig's text, K is looked up in the list of the letters' forward positions, the shifted text is
T[:K] + T[K + s:], it is cut into codons from codon K // 3 on and translated with a dictionary spelled out by amino acid, and the
letters of the first '*' are mapped back to transcript indices for the NMD rule.  Nothing here calls the library and nothing here
shares a segment search, a cursor or a bit trick with it."""
import functools

import numpy as np

import edit_cases as ed
from effects_cases import MITO, STANDARD, aa_table, code_string, masked  # noqa: F401  (the codes, spelled out by amino acid)
from helpers import revcomp

UNDEF = 0xFFFFFFFF
END, CAP, UNKNOWN = 0xFFFF, 0xFFFE, 0xFFFD
FLAGS = ("first", "last", "ptc1", "ptc2", "nmd1", "nmd2", "unknown")
FIRST, LAST, PTC1, PTC2, NMD1, NMD2, UNKNOWN_FLAG = (1 << k for k in range(7))
N_TX = 8  # transcripts 0 .. 6 have segments, transcript 7 has none

# (site_len, cut, nmd_window, start_window, max_codons): site_len 16, 23 and 32, cut 1 and site_len - 1, windows 0, 50 and 65535,
# max_codons 1 and 4096 - and the start windows 23 and 24, which the stop at transcript index 23 of transcript 0 meets and misses
SHAPES = {
    "SpCas9": (23, 17, 50, 0, 4096),
    "open": (23, 17, 0, 0, 4096),
    "never": (23, 17, 65535, 65535, 4096),
    "start23": (23, 17, 50, 23, 4096),
    "start24": (23, 17, 0, 24, 4096),
    "s16_first": (16, 1, 50, 0, 1),
    "s16_last": (16, 15, 50, 50, 4096),
    "s32_last": (32, 31, 50, 0, 4096),
    "s32_first": (32, 1, 0, 65535, 5),
    "cas12a": (23, 22, 50, 0, 2),
}
CODES = {"standard": STANDARD, "mito": MITO}


def _stop_free(rng, n):
    """n letters without T: no stop of the standard code in any frame"""
    return "".join("ACG"[k] for k in rng.integers(0, 3, n))


def _planted(rng, n, plants):
    text = list(_stop_free(rng, n))
    for at, letters in plants:
        text[at:at + len(letters)] = letters
    assert len(text) == n
    return "".join(text)


@functools.lru_cache(maxsize=None)
def small_genome():
    """(contigs, segments): about 1.5 kb.  segments = (contig, start, end, transcript, strand, phase) in (contig, start) order.
    The coding texts hold no T but the planted ones, so that the stops of the standard code fall where the cases need them
    (coding indices below are transcript indices, the shift included):
    0. transcript 0 on '+', phase 0, segments of 39, 36, 1 and 26 bases, introns of 2, 40 and 5: J = 76, E = 102.  Stops:
       TAA at 23 (frame 2; e = 26 = J - 50), T|AA at 38 (frame 2, split 1|2 over the first junction), TA|A at 73 (frame 1, split
       2|1 over the second junction, the A being the one-base segment; e = 76 = J), TAA at 80 (frame 2) and TAG at 85 (frame 1)
       in the last segment, behind which a walk reaches END, and the transcript's own TAA at 99.
    1. the reverse complement of 0 with transcript 1 on '-'
    2. 500 bases without a segment
    3. transcript 2 on '+', first phase 2 (shift 1), segments of 74 and 20 bases: J = 75, E = 95 (it ends in the middle of a
       codon).  Stops: TAA at 23 (frame 2; e = 26 = J - 49, and 23 - shift = 22), TGA at 40 (frame 1), TAA at 80 (frame 2).
       transcript 3 on '-', first phase 1 (shift 2), ONE segment of 40 bases: TAA at 10 (frame 1), TAG at 20 (frame 2).
    4. transcripts 4 ('+', 21 bases) and 5 ('-', 24 bases) in two abutting segments; transcript 6 on '+', phase 0, segments of 30
       and 40 bases, an N at 20, TAA at 10 (frame 1), TAA at 47 (frame 2), TGA at 55 (frame 1); it ends 8 bases in front of the
       contig's end, inside the genome's last word."""
    rng = np.random.default_rng(437)
    flank = lambda n: "".join("ACGT"[k] for k in rng.integers(0, 4, n))  # noqa: E731
    contigs, segments = [], []

    def place(contig, parts):
        """parts: texts and (text, transcript, strand, phase) tuples in forward order"""
        text = ""
        for part in parts:
            if isinstance(part, tuple):
                segments.append((contig, len(text), len(text) + len(part[0]), part[1], part[2], part[3]))
                part = part[0]
            text += part
        return text

    t0 = _planted(rng, 102, [(0, "ATGC"), (23, "TAA"), (38, "TAA"), (73, "TAA"), (80, "TAA"), (85, "TAG"), (99, "TAA")])
    contigs.append(place(0, [flank(45), (t0[:39], 0, 0, 0), flank(2), (t0[39:75], 0, 0, 0), flank(40), (t0[75:76], 0, 0, 0), flank(5),
                             (t0[76:], 0, 0, 2), flank(30)]))
    first = contigs[0]
    mirrored = [(len(first) - e, len(first) - s, 1, 1, ph) for c, s, e, _, _, ph in segments if c == 0]
    contigs.append(revcomp(first))
    segments.extend((1, s, e, tx, strand, ph) for s, e, tx, strand, ph in sorted(mirrored))
    contigs.append(flank(500))
    # (text offsets are coding indices less the shift)
    t2 = _planted(rng, 94, [(22, "TAA"), (39, "TGA"), (79, "TAA")])
    t3 = _planted(rng, 40, [(8, "TAA"), (18, "TAG")])
    contigs.append(place(3, [flank(40), (t2[:74], 2, 0, 2), flank(30), (t2[74:], 2, 0, 0), flank(35), (revcomp(t3), 3, 1, 1), flank(40)]))
    t6 = _planted(rng, 70, [(10, "TAA"), (20, "N"), (47, "TAA"), (55, "TGA")])
    contigs.append(place(4, [flank(40), (_stop_free(rng, 21), 4, 0, 0), (revcomp(_stop_free(rng, 24)), 5, 1, 0), flank(30),
                             (t6[:30], 6, 0, 0), flank(12), (t6[30:], 6, 0, 0), flank(8)]))
    return tuple(contigs), tuple(sorted(segments))


def every_locus(contigs):
    return ed.every_locus(contigs)


def invalid_loci(contigs):
    n, last = len(contigs), len(contigs) - 1
    length = len(contigs[last])
    return [(n, 0, 0), (0xFFFFFFFF, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1), (last, 10, 2), (last, 10, 0xFFFFFFFF), (last, length - 15, 0),
            (last, length - 15, 1), (last, 0xFFFFFFFF, 0), (0, 0xFFFFFFFF, 1), (last, 0xFFFFFFFF - 22, 0)]


# ---- the restatement --------------------------------------------------------------------------------------------------------
def transcripts_of(segments):
    """transcript -> (contig, strand, shift, its segments (start, end) in TRANSCRIPT order)"""
    out = {}
    for c, s, e, tx, strand, phase in sorted(segments):
        out.setdefault(tx, [c, strand, None, [], []])
        out[tx][3].append((s, e))
        out[tx][4].append(phase)
    for t in out.values():
        if t[1]:
            t[3].reverse()
            t[4].reverse()
        t[2] = (3 - t[4][0]) % 3
    return {tx: (t[0], t[1], t[2], tuple(t[3])) for tx, t in out.items()}


def coding_text(text, transcript):
    """(T, where): the transcript's text in transcript orientation with '?' for the `shift` indices in front of its first base,
    and the forward position of every letter (None for '?')"""
    _, strand, shift, segs = transcript
    letters, where = "?" * shift, [None] * shift
    for s, e in segs:
        piece = text[s:e]
        letters += revcomp(piece) if strand else piece
        where += list(range(e - 1, s - 1, -1)) if strand else list(range(s, e))
    return letters, where


def table_of(transcript):
    """(B_t, J_t or None without a junction) by hand: the bases of all segments, and shift + the bases of all but the last"""
    _, _, shift, segs = transcript
    lengths = [e - s for s, e in segs]
    return sum(lengths), (shift + sum(lengths[:-1]) if len(segs) > 1 else None)


def walk(shifted, origin, shift, codon, max_codons, table):
    """(d, first, e) of WALK over the shifted text from `codon` on; origin[j] = the transcript index of shifted letter j"""
    for n in range(max_codons):
        tri = shifted[3 * (codon + n):3 * (codon + n) + 3]
        if len(tri) < 3:
            return END, None, None
        if origin[3 * (codon + n)] < shift:
            continue
        if any(ch not in "ACGT" for ch in tri):
            return UNKNOWN, None, None
        if table[tri] == "*":
            return n, origin[3 * (codon + n)], origin[3 * (codon + n) + 2] + 1
    return CAP, None, None


def site_row(contigs, shown, txs, by_contig, locus, shape, table):
    """(row as four numbers, detail or None): detail = per frame (d, J_t - e or None, first - shift or None) for a coding cut.
    shown: the contigs' texts as the genome object holds them (masked)."""
    site_len, cut, nmd_window, start_window, max_codons = shape
    c, p, strand = locus
    if c >= len(contigs) or strand > 1 or p + site_len > len(contigs[c]):
        return (UNDEF,) * 4, None
    x = p + site_len - cut if strand else p + cut
    hit = [(s, e, tx) for s, e, tx in by_contig.get(c, ()) if s < x < e]
    if not hit:
        junction = any(s <= y < e for s, e, _ in by_contig.get(c, ()) for y in (x - 1, x))
        return (0xFFFFFFFF, 0, junction << 31, 0), None
    (start, end, tx), = hit
    t = txs[tx]
    _, t_strand, shift, segs = t
    T, where = coding_text(shown[c].upper(), t)
    K = where.index(x - 1 if t_strand else x)
    bases, junction_at = table_of(t)
    codon, frame = K // 3, K % 3
    frac = ((K - shift) * 65536) // bases
    edge = min(x - start, end - x, 255)
    flags = (FIRST if segs[0] == (start, end) else 0) | (LAST if segs[-1] == (start, end) else 0)
    ds, detail = [], []
    for s in (1, 2):
        shifted = T[:K] + T[K + s:]
        origin = list(range(K)) + list(range(K + s, len(T)))
        d, first, e = walk(shifted, origin, shift, codon, max_codons, table)
        ds.append(d)
        if d == UNKNOWN:
            flags |= UNKNOWN_FLAG
        if d < UNKNOWN:
            flags |= PTC1 << (s - 1)
            if junction_at is not None and junction_at - e >= nmd_window and (start_window == 0 or first - shift >= start_window):
                flags |= NMD1 << (s - 1)
            detail.append((d, None if junction_at is None else junction_at - e, first - shift))
        else:
            detail.append((d, None, None))
    return (tx, codon | frame << 30, frac | edge << 16 | flags << 24, ds[0] | ds[1] << 16), detail


def expected(contigs, segments, loci, shape, code=STANDARD, resident=None, n_tx=N_TX):
    """What a knock-out call gives for loci under shape = (site_len, cut, nmd_window, start_window, max_codons) and a code:
    {"rows": uint32[n, 4], "coverage": uint32[n_tx, 2], "stats", "detail": per locus None or the two frames' (d, J_t - e,
    first - shift)}.  resident: None or the half-open range of global positions the genome object holds."""
    table = aa_table(code)
    txs = transcripts_of(segments)
    off = ed.offsets(contigs)
    shown = [masked(t, off[c], resident) for c, t in enumerate(contigs)]
    by_contig = {}
    for c, s, e, tx, _, _ in segments:
        by_contig.setdefault(c, []).append((s, e, tx))
    rows = np.empty((len(loci), 4), dtype=np.uint32)
    stats = dict(defined=0, undefined=0, coding=0, junction=0, ptc=[0, 0], nmd=[0, 0], unknown=0, transcripts_covered=0)
    details, covered = [], {}
    for i, locus in enumerate(loci):
        row, detail = site_row(contigs, shown, txs, by_contig, tuple(int(v) for v in locus), shape, table)
        rows[i] = row
        details.append(detail)
        if row == (UNDEF,) * 4:
            stats["undefined"] += 1
            continue
        stats["defined"] += 1
        if detail is None:
            stats["junction"] += row[2] >> 31
            continue
        flags = row[2] >> 24
        stats["coding"] += 1
        for k in (0, 1):
            stats["ptc"][k] += bool(flags & PTC1 << k)
            stats["nmd"][k] += bool(flags & NMD1 << k)
        stats["unknown"] += bool(flags & UNKNOWN_FLAG)
        if flags & NMD1 and flags & NMD2:
            covered.setdefault(row[0], []).append(row[1] & 0x3FFFFFFF)
    coverage = np.zeros((n_tx, 2), dtype=np.uint32)
    coverage[:, 1] = UNDEF
    for tx, codons in covered.items():
        coverage[tx] = (len(codons), min(codons))
    stats["transcripts_covered"] = len(covered)
    return {"rows": rows, "coverage": coverage, "stats": stats, "detail": details}


def keep(row, limits):
    """FILTER for one expected row; limits = (min_frac, max_frac, min_edge, require, forbid) in the row's units."""
    min_frac, max_frac, min_edge, require, forbid = limits
    row = [int(w) for w in row]
    if row == [UNDEF] * 4 or row[0] == 0xFFFFFFFF:
        return False
    frac, edge, flags = row[2] & 0xFFFF, row[2] >> 16 & 0xFF, row[2] >> 24 & 0x7F
    return min_frac <= frac <= max_frac and edge >= min_edge and flags & require == require and not flags & forbid


def pick_column(rows):
    """The "knockout" pick column by hand: NMD in both frames first, then the smaller frac; no coding cut: 0."""
    out = []
    for row in rows:
        row = [int(w) for w in row]
        if row == [UNDEF] * 4 or row[0] == 0xFFFFFFFF:
            out.append(0)
        else:
            flags = row[2] >> 24
            out.append((65536 if flags & NMD1 and flags & NMD2 else 0) + 65535 - (row[2] & 0xFFFF))
    return np.array(out, dtype=np.uint64)


def occurrences(contigs, segments):
    """Asserts, from the restatement alone, that the small genome holds what the tests are for: every flag bit, END, CAP,
    UNKNOWN and JUNCTION, NMD1 != NMD2, a PTC with J_t - e equal to nmd_window (NMD) and to nmd_window - 1 (not), a first index
    equal to start_window (NMD) and one below it (not), max_codons equal to d + 1 (PTC) and to d (CAP), a PTC in a last
    segment, breaks in all three frames, and stops split 1|2 and 2|1 over junctions."""
    loci = every_locus(contigs)
    seen_flags, seen_d, frames = 0, set(), set()
    junction = differ = last_ptc = False
    at_window = below_window = at_start = below_start = False
    for name in ("SpCas9", "start23", "start24", "s16_first", "cas12a"):
        shape = SHAPES[name]
        want = expected(contigs, segments, loci, shape)
        nmd_window, start_window, max_codons = shape[2:]
        at_cap = below_cap = False
        plain = expected(contigs, segments, loci, shape[:4] + (4096,))["detail"] if max_codons < 4096 else want["detail"]
        for row, detail, far in zip(want["rows"], want["detail"], plain):
            row = [int(w) for w in row]
            if detail is None:
                junction |= row[0] == 0xFFFFFFFF and row[2] >> 31 == 1
                continue
            flags = row[2] >> 24
            seen_flags |= flags
            frames.add(row[1] >> 30)
            differ |= bool(flags & NMD1) != bool(flags & NMD2)
            for k, (d, room, first) in enumerate(detail):
                seen_d.add(d if d >= UNKNOWN else "ptc")
                nmd = bool(flags & NMD1 << k)
                if d < UNKNOWN:
                    last_ptc |= bool(flags & LAST)
                    if room is not None and (start_window == 0 or first >= start_window):
                        at_window |= room == nmd_window and nmd
                        below_window |= room == nmd_window - 1 and not nmd
                    if room is not None and room >= nmd_window and start_window:
                        at_start |= first == start_window and nmd
                        below_start |= first == start_window - 1 and not nmd
                    at_cap |= d + 1 == max_codons
                below_cap |= d == CAP and far[k][0] == max_codons
        if max_codons < 4096:
            assert at_cap and below_cap, (name, at_cap, below_cap)
    assert at_window and below_window and at_start and below_start, (at_window, below_window, at_start, below_start)
    assert seen_flags == 0x7F, hex(seen_flags)
    assert seen_d == {"ptc", END, CAP, UNKNOWN}, seen_d
    assert frames == {0, 1, 2} and junction and differ and last_ptc
    # the split stops of transcript 0: their letters lie in two segments
    txs = transcripts_of(segments)
    T, where = coding_text(contigs[0], txs[0])
    assert T[38:41] == "TAA" and where[39] - where[38] > 1 and where[40] - where[39] == 1
    assert T[73:76] == "TAA" and where[74] - where[73] == 1 and where[75] - where[74] > 1

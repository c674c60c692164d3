"""Shared helpers of test_effects.py (GPU) and test_effects_cpu.py: the definition of the coding consequences of base edits
(include/varscot_hip.h: CODE, SEGMENT, CODING, CODON, PARAMS, EFFECT, ROW, COVERAGE, FILTER) in plain Python on strings, and the
small genome of the tests.  A different formulation from the library's walk: the contig's text is MUTATED at the candidate's
converted forward positions, every transcript's coding string is rebuilt from both texts by slicing and reverse-complementing,
both strings are cut into codons and translated with a dictionary spelled out by amino acid, and the codons that differ are the
effects.  Nothing here calls the library and nothing here shares a coding index, a segment search or a bit trick with it."""
import functools

import numpy as np

import edit_cases as ed
import varscot_amd as va
from helpers import random_seq, revcomp

CLASSES = ed.CLASSES
EFFECTS = ("synonymous", "missense", "stop_gained", "stop_lost", "start_lost", "unknown")
UNDEF = 0xFFFFFFFF
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}

# the standard genetic code, by amino acid
STANDARD = {
    "A": "GCT GCC GCA GCG", "R": "CGT CGC CGA CGG AGA AGG", "N": "AAT AAC", "D": "GAT GAC", "C": "TGT TGC", "Q": "CAA CAG",
    "E": "GAA GAG", "G": "GGT GGC GGA GGG", "H": "CAT CAC", "I": "ATT ATC ATA", "L": "TTA TTG CTT CTC CTA CTG", "K": "AAA AAG",
    "M": "ATG", "F": "TTT TTC", "P": "CCT CCC CCA CCG", "S": "TCT TCC TCA TCG AGT AGC", "T": "ACT ACC ACA ACG", "W": "TGG",
    "Y": "TAT TAC", "V": "GTT GTC GTA GTG", "*": "TAA TAG TGA",
}
# the vertebrate mitochondrial code: AGA and AGG stop, ATA is M, TGA is W
MITO = dict(STANDARD, R="CGT CGC CGA CGG", I="ATT ATC", M="ATG ATA", W="TGG TGA")
MITO["*"] = "TAA TAG AGA AGG"


def aa_table(by_amino_acid):
    """codon -> amino-acid letter"""
    table = {codon: aa for aa, codons in by_amino_acid.items() for codon in codons.split()}
    assert len(table) == 64
    return table


def code_string(by_amino_acid):
    """The 64 letters of a code in the library's order: first base slowest, A C G T."""
    table = aa_table(by_amino_acid)
    return "".join(table[a + b + c] for a in "ACGT" for b in "ACGT" for c in "ACGT")


def codon_number(text):
    return 16 * "ACGT".index(text[0]) + 4 * "ACGT".index(text[1]) + "ACGT".index(text[2])


# ---- the small genome -------------------------------------------------------------------------------------------------------
N_TX = 11  # transcripts 0 .. 9 have segments, transcript 10 has none


@functools.lru_cache(maxsize=None)
def small_genome():
    """(contigs, segments): about 1.1 kb.  segments = (contig, start, end, transcript, strand, phase) in (contig, start) order.
    1. a '+' transcript of four segments - ATG CAA T|GG CAG CG|A|CCA GGC TGG CAA ACC CCC GGG TAA - whose codons are split 1|2
       and 2|1 over junctions, one segment a single base, introns of 2 (both parts of TGG lie in one window), 40 and 5 bases
    2. the reverse complement of 1 with the same transcript on '-'
    3. transcripts whose first phase is 1 ('+') and 2 ('-'), and one that ends in the middle of a codon
    4. a transcript whose codon CAA is split 2|1 over an intron in which the 3-base segment of another transcript lies
    5. a segment at base 0, a segment with an N inside a codon, a segment that ends at the contig's end
    6. 500 random bases without a segment"""
    rng = np.random.default_rng(429)
    flank = lambda n: random_seq(rng, n)  # noqa: E731
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

    # (45 bases in front: the single base then lies at 101, behind the first three words, and the two other bases of its codon in
    # front of them - a codon whose bases an object without those words holds in part)
    one = [flank(45), ("ATGCAAT", 0, 0, 0), flank(2), ("GGCAGCG", 0, 0, 2), flank(40), ("A", 0, 0, 1), flank(5),
           ("CCAGGCTGGCAAACCCCCGGGTAA", 0, 0, 0), flank(30)]
    contigs.append(place(0, one))
    first = contigs[0]
    mirrored = [(len(first) - e, len(first) - s, 1, 1, ph) for c, s, e, _, _, ph in segments if c == 0]
    contigs.append(revcomp(first))
    segments.extend((1, s, e, tx, strand, ph) for s, e, tx, strand, ph in sorted(mirrored))
    contigs.append(place(2, [flank(30), ("GCAATGGCGACAGC", 2, 0, 1), flank(25), (revcomp("GGCAATGGCGATAG"), 3, 1, 2), flank(25),
                             ("ATGCAATGGCA", 4, 0, 0), flank(30)]))
    contigs.append(place(3, [flank(30), ("ATGC", 5, 0, 0), flank(10), ("ATGCA", 6, 0, 0), flank(8), ("AGG", 5, 0, 2), flank(9),
                             ("ATGGCGATAA", 6, 0, 1), flank(30)]))
    contigs.append(place(4, [("ATGCAATGGCAG", 7, 0, 0), flank(35), ("ATGCNATGGCAA", 8, 0, 0), flank(35), ("ATGCAATGGTAA", 9, 0, 0)]))
    contigs.append(flank(500))
    return tuple(contigs), tuple(sorted(segments))


def random_cds(rng, contigs, gap=(20, 200), length=(30, 150), per_transcript=3):
    """Exon-like segments over contigs, (segments, n_tx): gaps and lengths drawn from the ranges, every `per_transcript`
    consecutive segments of a contig one transcript on a random strand with a random first phase, the later phases made to
    continue the reading frame."""
    segments, tx = [], 0
    for c, text in enumerate(contigs):
        at, mine = int(rng.integers(*gap)), []
        while at + length[1] < len(text):
            n = int(rng.integers(*length))
            mine.append((at, at + n))
            at += n + int(rng.integers(*gap))
        for k in range(0, len(mine), per_transcript):
            group = mine[k:k + per_transcript]
            strand, phase = int(rng.integers(0, 2)), int(rng.integers(0, 3))
            ci = (3 - phase) % 3
            for j, (s, e) in enumerate(group[::-1] if strand else group):
                segments.append((c, s, e, tx, strand, phase if j == 0 else (3 - ci % 3) % 3))
                ci += e - s
            tx += 1
    return tuple(sorted(segments)), tx


def every_locus(contigs):
    return ed.every_locus(contigs)


def invalid_loci(contigs):
    n, last = len(contigs), len(contigs) - 1
    length = len(contigs[last])
    return [(n, 0, 0), (0xFFFFFFFF, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 1), (last, 10, 2), (last, 10, 0xFFFFFFFF), (last, length - 15, 0),
            (last, length - 15, 1), (last, 0xFFFFFFFF, 0), (0, 0xFFFFFFFF, 1), (last, 0xFFFFFFFF - 22, 0)]


# ---- the restatement --------------------------------------------------------------------------------------------------------
def transcripts_of(segments):
    """transcript -> (contig, strand, first phase, its segments in TRANSCRIPT order)"""
    out = {}
    for c, s, e, tx, strand, phase in sorted(segments):
        out.setdefault(tx, [c, strand, None, []])[3].append((s, e, phase))
    for tx, t in out.items():
        if t[1]:
            t[3].reverse()
        t[2] = t[3][0][2]
    return out


def coding(text, transcript):
    """(the transcript's coding string out of a contig's text with '?' in front for the bases its first codon lacks and behind
    for those its last one lacks, the forward position of every letter or None)"""
    _, strand, phase, segs = transcript
    letters, where = "?" * ((3 - phase) % 3), [None] * ((3 - phase) % 3)
    for s, e, _ in segs:
        piece = text[s:e]
        letters += revcomp(piece) if strand else piece
        where += list(range(e - 1, s - 1, -1)) if strand else list(range(s, e))
    pad = -len(letters) % 3
    return letters + "?" * pad, where + [None] * pad


def masked(text, contig_offset, resident):
    """A contig's text with 'n' where the genome object does not hold the base."""
    if resident is None:
        return text
    return "".join(ch if resident[0] <= contig_offset + i < resident[1] else "n" for i, ch in enumerate(text))


def classify(ref, alt, codon, first_phase, table):
    """The class of an effect by the rules in their order; ref, alt: three letters each."""
    if any(ch not in "ACGT" for ch in ref):
        return "unknown"
    if codon == 0 and first_phase == 0:
        return "start_lost"
    if table[ref] != "*" and table[alt] == "*":
        return "stop_gained"
    if table[ref] == "*" and table[alt] != "*":
        return "stop_lost"
    return "synonymous" if table[ref] == table[alt] else "missense"


def raw_effects(contigs, segments, loci, shape, to, resident=None):
    """Per locus: None where the site is not defined, else (class "defined", window positions of the editor's base, those of
    them inside a segment, [(lowest forward edited position, transcript, codon, ref letters, alt letters, edited bases, at,
    first phase)] in the order of the definition).  The class of the site comes back beside it."""
    site_len, start, length, base = shape
    txs = transcripts_of(segments)
    off = ed.offsets(contigs)
    covered = {}
    for c, s, e, *_ in segments:
        covered.setdefault(c, set()).update(range(s, e))
    shown = {c: masked(t, off[c], resident) for c, t in enumerate(contigs)}
    out = []
    for locus in loci:
        cls, text = ed.site_of(contigs, locus, site_len, resident)
        if cls != "defined":
            out.append((cls, None, None, None))
            continue
        c, p, strand = locus
        window = text[start:start + length]
        at = [j for j in range(length) if window[j] == base]
        forward = {(p + site_len - 1 - (start + j) if strand else p + start + j): j for j in at}
        inside = sorted(j for f, j in forward.items() if f in covered.get(c, ()))
        effects = []
        if inside:
            mutated = list(shown[c])
            for f in forward:
                assert mutated[f] == (COMP[base] if strand else base)
                mutated[f] = COMP[to] if strand else to
            mutated = "".join(mutated)
            for tx, t in sorted(txs.items()):
                if t[0] != c or not any(s <= f < e for f in forward for s, e, _ in t[3]):
                    continue  # (no letter of this transcript changes)
                before, where = coding(shown[c], t)
                after, _ = coding(mutated, t)
                for k in range(len(before) // 3):
                    ref, alt = before[3 * k:3 * k + 3], after[3 * k:3 * k + 3]
                    changed = [where[3 * k + i] for i in range(3) if ref[i] != alt[i]]
                    if changed:
                        effects.append((min(changed), tx, k, ref, alt, len(changed), min(forward[f] for f in changed), t[2]))
            effects.sort()
        out.append((cls, at, inside, effects))
    return out


def expected(contigs, segments, loci, shape, to, code=STANDARD, resident=None, n_tx=N_TX, raw=None):
    """What an effects call gives for loci under shape = (site_len, win_start, win_len, base letter), `to` (a letter) and a
    code: {"rows": uint32[n, 2], "effects": EFFECT_DTYPE, "coverage": uint32[n_tx, 2], "stats", "classes": per locus the set of
    its effects' class indices or None, "frames": {(transcript, frame of the emitting base)}}.  raw: raw_effects' result for
    the same arguments (it does not depend on the code)."""
    table = aa_table(code)
    raw = raw if raw is not None else raw_effects(contigs, segments, loci, shape, to, resident)
    rows = np.empty((len(loci), 2), dtype=np.uint32)
    stats = dict.fromkeys(CLASSES, 0)
    stats.update(with_effect=0, effects=0, transcripts_stopped=0, by_class=dict.fromkeys(EFFECTS, 0))
    records, classes = [], []
    stops = {}
    for i, (cls, at, inside, effects) in enumerate(raw):
        stats[cls] += 1
        if cls != "defined":
            rows[i] = (UNDEF, UNDEF)
            classes.append(None)
            continue
        word0, mine = 0, set()
        for _, tx, k, ref, alt, n_changed, j, first_phase in effects:
            name = classify(ref, alt, k, first_phase, table)
            e = EFFECTS.index(name)
            stats["by_class"][name] += 1
            word0 += 32 ** e
            mine.add(e)
            r, a = (0, 0) if name == "unknown" else (codon_number(ref), codon_number(alt))
            records.append((i, tx, k, r + 64 * a + 4096 * e + 65536 * n_changed + 1048576 * j))
            if name == "stop_gained":
                stops.setdefault(tx, []).append(k)
        rows[i] = (word0, ed.number(inside))
        classes.append(mine)
        stats["with_effect"] += bool(effects)
    out = np.zeros(len(records), dtype=va.EFFECT_DTYPE)
    for n, rec in enumerate(records):
        out[n] = rec
    stats["effects"] = len(records)
    coverage = np.zeros((n_tx, 2), dtype=np.uint32)
    coverage[:, 1] = UNDEF
    for tx, codons in stops.items():
        coverage[tx] = (len(codons), min(codons))
    stats["transcripts_stopped"] = len(stops)
    return {"rows": rows, "effects": out, "coverage": coverage, "stats": stats, "classes": classes}


def keep(classes, require, forbid):
    """FILTER for one expected candidate: classes = the set of its effects' class indices or None; require, forbid: class names."""
    if classes is None:
        return False
    req = {EFFECTS.index(c) for c in require}
    forb = {EFFECTS.index(c) for c in forbid}
    return (not req or bool(classes & req)) and not classes & forb


def split_frames(contigs, segments, raw):
    """{(transcript strand, frame)} over the effects of `raw` whose codon is split over two segments, the frame being that of
    the emitting base (the codon's lowest-forward edited base)."""
    txs = transcripts_of(segments)
    seen = set()
    for _, _, _, effects in raw:
        for low, tx, k, _, _, _, _, _ in effects or ():
            t = txs[tx]
            _, where = coding(contigs[t[0]], t)
            places = [w for w in where[3 * k:3 * k + 3] if w is not None]
            if len(places) == 3 and max(places) - min(places) > 2:
                seen.add((t[1], where.index(low) % 3))
    return seen

"""The definition of HDR knock-in design (include/varscot_hip.h) restated on strings: the context by slicing and
reverse complement, E and S as Python strings, the rules letter by letter, ALLOWED by translating codons of the contig text.
Nothing here calls the library; tests/test_hdr_cpu.py and tests/test_hdr.py compare the library against it bit for bit."""
import bisect

import numpy as np

import varscot_amd as va

UNDEF = 0xFFFFFFFF
CLASSES = ("defined", "invalid", "off_contig", "not_resident", "has_n")
B_PAM, B_SEED, B_PROTO, SUB_PAM, SUB_SEED, OPEN = 1, 2, 4, 8, 16, 32
SUBSTITUTE, F_SUB_SEED, F_NONCODING = 1, 2, 4
LETTERS = "ACGT"
CODE = va.GENETIC_CODE
# a code that is not the standard one: the vertebrate mitochondrial table (AGA / AGG stop, ATA Met, TGA Trp)
OTHER_CODE = "".join({"AGA": "*", "AGG": "*", "ATA": "M", "TGA": "W"}.get(a + b + c, CODE[16 * i + 4 * j + k])
                     for i, a in enumerate(LETTERS) for j, b in enumerate(LETTERS) for k, c in enumerate(LETTERS))


def revcomp(s):
    return s.translate(str.maketrans("ACGT", "TGCA"))[::-1]


SHAPES = {
    "SpCas9": va.HDR_NUCLEASES["SpCas9"],
    "Cas12a": va.HDR_NUCLEASES["Cas12a"],
    # site_len 16 with no context around it, the cut at 1, every edit of the context in reach, one seed mismatch blocks
    "bare16": va.HdrShape(16, 0, 0, 1, 63, 1, (13, "NGG"), (5, 8), (0, 13), 1, 2),
    # site_len 32 with 32 bases in front and none behind, the cut at site_len - 1
    "front32": va.HdrShape(32, 32, 0, 31, 63, 0, (0, "TTTV"), (4, 16), (4, 28), 2, 4),
    "dist0": va.HdrShape(23, 20, 21, 17, 0, 1, (20, "NGG"), (10, 10), (0, 20), 2, 4),
    "seed1": va.HdrShape(23, 20, 21, 17, 30, 1, (20, "NGG"), (10, 10), (0, 20), 1, 4),
    # both anchors with the PAM at the far end of the site
    "far1": va.HdrShape(20, 10, 12, 3, 25, 1, (0, "CCN"), (3, 8), (3, 17), 1, 3),
    "far0": va.HdrShape(24, 8, 8, 20, 25, 0, (21, "NGG"), (11, 10), (0, 21), 2, 0),
    "nosub": va.HdrShape(23, 20, 21, 17, 30, 1, (20, "NGG"), (10, 10), (0, 20), 2, 4, substitute=False, sub_seed=False, sub_noncoding=False),
    # SUBSTITUTE without SUB_SEED and without SUB_NONCODING, no seed or protospacer rule, an empty PAM
    "pamonly": va.HdrShape(23, 20, 21, 17, 30, 1, (20, "NGG"), (10, 10), (0, 20), 0, 0, sub_seed=False, sub_noncoding=False),
    "nopam": va.HdrShape(23, 20, 21, 17, 30, 1, (23, ""), (10, 10), (0, 20), 1, 4),
}


def shape_of(name):
    return SHAPES[name]


# ---- one context, one edit in read coordinates ------------------------------------------------------------------------------------
def pair_text(R, sh, e0, del_len, I, allowed):
    """The pair of context R (read orientation) with the edit that replaces R[e0, e0 + del_len) by I: None when it is not in reach,
    else (info, block, edited, seen) - seen: the things the tests want to have met.  allowed(r, b) -> (ok, coding)."""
    C_, s0, L = len(R), sh.up, sh.site_len
    assert C_ == sh.context_len
    K, e1 = s0 + sh.cut, e0 + del_len
    if e0 <= K <= e1:
        dist, side = 0, 0
    elif e1 < K:
        dist, side = K - e1, 1
    else:
        dist, side = e0 - K, 2
    if dist > sh.max_dist:
        return None
    E = R[:e0] + I + R[e1:]
    delta = len(I) - del_len
    moved = e0 < s0 + L if sh.anchor == 1 else e1 <= s0
    shift = delta if moved else 0
    seen = set()

    def at(q):
        x = s0 + q + shift
        if x < 0:
            seen.add("no_letter_front")
        if x >= len(E):
            seen.add("no_letter_back")
        return E[x] if 0 <= x < len(E) else None

    S = [at(q) for q in range(L)]
    pam_broken = any(S[sh.pam_start + j] is None or not sh.pam_accept[j] >> LETTERS.index(S[sh.pam_start + j]) & 1 for j in range(sh.pam_len))
    seed_mm = sum(S[q] != R[s0 + q] for q in range(sh.seed_start, sh.seed_start + sh.seed_len))
    proto_mm = sum(S[q] != R[s0 + q] for q in range(sh.proto_start, sh.proto_start + sh.proto_len))
    flags = (B_PAM if pam_broken else 0) | (B_SEED if sh.min_seed_mm and seed_mm >= sh.min_seed_mm else 0) \
        | (B_PROTO if sh.min_proto_mm and proto_mm >= sh.min_proto_mm else 0)
    block = UNDEF
    edited = E
    if not flags:
        found = None

        def slot(q):
            x = s0 + q + shift
            if not 0 <= x < len(E) or e0 <= x < e0 + len(I):
                return None
            return x, (x if x < e0 else x - delta)

        if sh.flags & SUBSTITUTE:
            for j in range(sh.pam_len):
                q = sh.pam_start + j
                if found or slot(q) is None:
                    continue
                x, r = slot(q)
                for b in range(4):
                    ok, coding = allowed(r, b)
                    if not sh.pam_accept[j] >> b & 1 and ok:
                        found = (SUB_PAM, q, b, coding, r, x)
                        break
            if not found and sh.flags & F_SUB_SEED and sh.min_seed_mm and seed_mm + 1 >= sh.min_seed_mm:
                qs = range(sh.seed_start, sh.seed_start + sh.seed_len)
                for q in (reversed(qs) if sh.anchor == 1 else qs):
                    if found or slot(q) is None or S[q] != R[s0 + q]:
                        continue
                    x, r = slot(q)
                    for b in range(4):
                        ok, coding = allowed(r, b)
                        if LETTERS[b] != R[s0 + q] and ok:
                            found = (SUB_SEED, q, b, coding, r, x)
                            break
        if found:
            flags, q, b, coding, r, x = found
            block = q | b << 8 | int(coding) << 10 | r << 16
            edited = E[:x] + LETTERS[b] + E[x + 1:]
        else:
            flags = OPEN
    info = dist | side << 6 | seed_mm << 8 | proto_mm << 13 | flags << 24
    return info, block, edited, seen


def allowed_from_sets(sets):
    """ALLOWED of vsc_hdr_site_text's letter sets (None: always); there is no CDS, so nothing is coding."""
    return lambda r, b: (True if sets is None else bool(sets[r] >> b & 1), 0)


# ---- genomes, loci, edits, CDS -------------------------------------------------------------------------------------------------------
def small_genome(site_len, C_, seed=11):
    """Contigs of site_len - 1, C - 1, C, C + 1, of 400 bases with an N run, and two of 200 bases that lie one N apart."""
    rng = np.random.default_rng(seed)

    def seq(n):
        return "".join(LETTERS[i] for i in rng.integers(0, 4, n))
    long = seq(400)
    long = long[:150] + "N" * 7 + long[157:]
    pair = seq(200) + "N" + seq(200)
    return [seq(site_len - 1), seq(C_ - 1), seq(C_), seq(C_ + 1), long, pair[:200], pair[201:]]


def every_locus(contigs):
    return [(c, p, s) for c, t in enumerate(contigs) for p in range(len(t) + 1) for s in (0, 1)]


def invalid_loci(contigs):
    n = len(contigs)
    return [(n, 0, 0), (0xFFFFFFFF, 5, 1), (4, 10, 2), (4, 0xFFFFFFFF, 0), (4, len(contigs[4]) + 1, 1), (2, 0x80000000, 0)]


def locus_array(loci):
    a = np.zeros(len(loci), dtype=va.LOCUS_DTYPE)
    for i, (c, p, s) in enumerate(loci):
        a[i] = (c, p, s, 0)
    return a


def other_letter(ch, k=1):
    return LETTERS[(LETTERS.index(ch) + k) % 4] if ch in LETTERS else "A"


def edit_sets(contigs, seed=5):
    """none, an SNV at every position, and insertions, deletions and replacements of 1 to 16 letters in turn - at every contig's
    first base and an insertion at pos = length among them."""
    rng = np.random.default_rng(seed)
    snv = [(c, p, 1, other_letter(t[p], 1 + (p % 3))) for c, t in enumerate(contigs) for p in range(len(t))]
    indel = []
    k = 0
    for c, t in enumerate(contigs):
        p = 0
        while p <= len(t):
            n = 1 + k % 16
            kind = k % 3
            ins = "".join(LETTERS[i] for i in rng.integers(0, 4, n)) if kind != 1 else ""
            del_len = min(n if kind != 0 else 0, len(t) - p)
            if p == len(t) or (del_len == 0 and not ins):
                del_len, ins = 0, ins or "G"
            indel.append((c, p, del_len, ins))
            p += (1 + k % 7) if p < len(t) - 9 else 1 + del_len
            k += 1
        if indel[-1][1] != len(t):
            indel.append((c, len(t), 0, "TAG"))
    order = np.random.default_rng(seed + 1).permutation(len(indel))
    mixed = [indel[i] for i in order]
    return {"none": None, "snv": snv, "indel": mixed, "few": mixed[::5]}  # few: most candidates reach one or two of them, some none


def cds_segments(contigs):
    """Transcripts on both strands over the 400-base contig and the two 200-base ones: segments of one and two bases, codons
    split over junctions, first phases other than 0, and one transcript that is too short for its last codon."""
    seg = [
        # transcript 0, '+', phase 0: exons of 10, 1, 2 and 20 bases
        (4, 20, 30, 0, 0, 0), (4, 33, 34, 0, 0, 2), (4, 40, 42, 0, 0, 1), (4, 50, 70, 0, 0, 2),
        # transcript 1, '-', its first (rightmost) segment has phase 1; it runs into the N run
        (4, 140, 153, 1, 1, 0), (4, 160, 171, 1, 1, 2), (4, 180, 200, 1, 1, 1),
        # transcript 2, '+', phase 2, one long exon
        (4, 230, 330, 2, 0, 2),
        # transcript 3, '-', phase 0, two exons with a 2-base one between them
        (5, 10, 61, 3, 1, 2), (5, 70, 72, 3, 1, 1), (5, 80, 130, 3, 1, 0),
        # transcript 4, '+', covers a whole contig
        (6, 0, 200, 4, 0, 0),
    ]
    assert all(e <= len(contigs[c]) for c, _, e, _, _, _ in seg)
    return seg


class CodingMap:
    """ALLOWED against a CDS from the contig text: per forward base its transcript's strand and the three forward positions of
    its codon (None where the transcript has no such base)."""

    def __init__(self, contigs, segments, code=None):
        self.contigs, self.code = contigs, code or CODE
        self.at = {}
        by_tx = {}
        for c, s, e, tx, strand, phase in segments:
            by_tx.setdefault(tx, []).append((c, s, e, strand, phase))
        for tx, segs in by_tx.items():
            strand = segs[0][3]
            segs = sorted(segs, key=lambda g: g[1], reverse=bool(strand))
            shift = (3 - segs[0][4]) % 3
            pos = []
            for c, s, e, _, _ in segs:
                pos += [(c, p) for p in (range(e - 1, s - 1, -1) if strand else range(s, e))]
            where = {shift + k: cp for k, cp in enumerate(pos)}
            for ci, cp in where.items():
                codon = ci // 3
                self.at[cp] = (strand, [where.get(3 * codon + i) for i in range(3)], ci % 3)

    def allowed(self, contig, f, fb, e_pos, del_len, noncoding_ok):
        """(ok, coding) of writing forward letter fb at forward position f of `contig`, beside the edit at e_pos."""
        if (contig, f) not in self.at:
            return noncoding_ok, 0
        strand, codon, i = self.at[(contig, f)]
        if any(cp is None for cp in codon):
            return False, 1
        if any(e_pos <= g + 1 and g <= e_pos + del_len for _, g in codon):
            return False, 1
        ref = [self.contigs[c][g] for c, g in codon]
        if any(ch not in LETTERS for ch in ref):
            return False, 1
        if strand:
            ref = [revcomp(ch) for ch in ref]
        alt = list(ref)
        alt[i] = revcomp(LETTERS[fb]) if strand else LETTERS[fb]

        def aa(cod):
            return self.code[16 * LETTERS.index(cod[0]) + 4 * LETTERS.index(cod[1]) + LETTERS.index(cod[2])]
        return aa(ref) == aa(alt), 1


def context_of(contigs, sh, contig, pos, strand, resident=None):
    """(class, R, F0) of a locus; resident = (first, end) global positions an object holds (None: everything)."""
    if contig >= len(contigs) or strand > 1:
        return 1, None, None
    t = contigs[contig]
    if pos > len(t) or len(t) - pos < sh.site_len:
        return 1, None, None
    left, right = (sh.down, sh.up) if strand else (sh.up, sh.down)
    if pos < left or len(t) - pos - sh.site_len < right:
        return 2, None, None
    f0 = pos - left
    if resident is not None:
        g = offsets(contigs)[contig] + f0
        if g < resident[0] or g + sh.context_len > resident[1]:
            return 3, None, None
    text = t[f0:f0 + sh.context_len]
    if "N" in text:
        return 4, None, None
    return 0, (revcomp(text) if strand else text), f0


def offsets(contigs):
    off, o = [], 0
    for t in contigs:
        off.append(o)
        o += len(t) + 1
    return off


def expected(contigs, loci, sh, edits, coding=None, resident=None):
    """rows, pairs (edit = the index in `edits` as given), coverage and the stats' counts of a call over `loci`."""
    n_e = 0 if edits is None else len(edits)
    rows = np.zeros((len(loci), 2), dtype=np.uint32)
    pairs = []
    by_contig = {}
    for k, (c, p, d, ins) in enumerate(edits or []):
        by_contig.setdefault(c, []).append((p, d, ins, k))
    for v in by_contig.values():
        v.sort()
    cls_count = [0] * 5
    C_ = sh.context_len
    seen = set()
    for i, (c, p, s) in enumerate(loci):
        cls, R, f0 = context_of(contigs, sh, c, p, s, resident)
        cls_count[cls] += 1
        if cls:
            rows[i] = (UNDEF, UNDEF)
            continue
        n_pairs = n_usable = 0
        mine = by_contig.get(c, [])
        for e_pos, d, ins, k in mine[bisect.bisect_left(mine, (f0,)):]:  # (ascending positions: a shortcut of the walk, not a rule)
            if e_pos > f0 + C_:
                break
            if not (f0 <= e_pos and e_pos + d <= f0 + C_):
                continue
            e0 = C_ - (e_pos - f0) - d if s else e_pos - f0
            I = revcomp(ins) if s else ins

            def allowed(r, b, e_pos=e_pos, d=d):
                if coding is None:
                    return True, 0
                f = f0 + (C_ - 1 - r if s else r)
                return coding.allowed(c, f, 3 - b if s else b, e_pos, d, bool(sh.flags & F_NONCODING))
            got = pair_text(R, sh, e0, d, I, allowed)
            if got is None:
                continue
            info, block = got[0], got[1]
            seen |= got[3]
            pairs.append((i, k, info, block))
            n_pairs += 1
            n_usable += not info >> 24 & OPEN
        rows[i] = (n_pairs, n_usable)
    pr = np.array(pairs, dtype=va.HDR_PAIR_DTYPE) if pairs else np.zeros(0, dtype=va.HDR_PAIR_DTYPE)
    pr = pr[np.lexsort((pr["edit"], pr["candidate"]))]
    cov = np.zeros((n_e, 2), dtype=np.uint32)
    cov[:, 1] = UNDEF
    for _, k, info, _ in pairs:
        if not info >> 24 & OPEN:
            cov[k, 0] += 1
            cov[k, 1] = min(int(cov[k, 1]), info & 63)
    defined = rows[:, 0] != UNDEF
    stats = dict(zip(CLASSES, cls_count))
    stats.update(with_pair=int((defined & (rows[:, 0] > 0)).sum()), with_usable=int((defined & (rows[:, 1] > 0)).sum()), pairs=len(pairs),
                 edits_covered=int((cov[:, 0] > 0).sum()), pairs_by_flag=[int(sum(info >> (24 + b) & 1 for _, _, info, _ in pairs)) for b in range(6)])
    return {"rows": rows, "pairs": pr, "coverage": cov, "stats": stats, "seen": seen}


def keep(row, have_edits, allow_open):
    """FILTER of one row."""
    if int(row[0]) == UNDEF and int(row[1]) == UNDEF:
        return False
    return (not have_edits) or row[1] >= 1 or (allow_open and row[0] >= 1)

"""Shared helpers of test_fold.py (GPU) and test_fold_cpu.py: the definition of the guide RNA's self-complementarity
(include/varscot_hip.h: SHAPE, SCAFFOLD, SPACER, PAIR, SELF STEM, SCAFFOLD STEM, QUAL, COVERED, ROW, FILTER) restated on STRINGS
- pairing by a dictionary, stems by slicing and all(), COVERED as a Python set - the shapes, the planted case families and the
small genome of the tests.  Nothing here forms a mask or walks a diagonal and nothing here calls the library: that the library's
diagonal form gives what the stems give is what the tests test."""
import collections
import functools

import numpy as np

import varscot_amd as va
from helpers import random_seq, revcomp

CLASSES = ("defined", "invalid", "off_contig", "not_resident", "has_n")
UNDEF = 0xFFFFFFFF
NO_LIMIT = 0xFFFFFFFF
WOBBLE = 1

Shape = collections.namedtuple("Shape", "site_len proto_start proto_len stem gc_min min_loop seed_start seed_len flags")

COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def va_shape(s, validate=True):
    return va.FoldShape(s.site_len, (s.proto_start, s.proto_len), s.stem, s.gc_min, s.min_loop, (s.seed_start, s.seed_len), flags=s.flags,
                        validate=validate)


def letters(text):
    """Upper case, U read as T."""
    return text.upper().replace("U", "T")


def pair(a, b, wobble):
    return COMPLEMENT[a] == b or (wobble and {a, b} == {"G", "T"})


def self_stem(g, i, j, L, min_loop, wobble):
    """SELF STEM (i, j, L), literally."""
    return 0 <= i and i + L + min_loop <= j and j + L <= len(g) and all(pair(a, b, wobble) for a, b in zip(g[i:i + L], reversed(g[j:j + L])))


def scaffold_stem(g, s, i, j, L, wobble):
    """SCAFFOLD STEM (i, j, L), literally."""
    return 0 <= i and 0 <= j and i + L <= len(g) and j + L <= len(s) and all(pair(a, b, wobble) for a, b in zip(g[i:i + L], reversed(s[j:j + L])))


def qual(g, i, shape):
    return sum(ch in "GC" for ch in g[i:i + shape.stem]) >= shape.gc_min


def stems(g, s, shape):
    """(self stems (i, j) of length k, scaffold stems (i, j) of length k) - every one, qualified or not."""
    n, k, w = len(g), shape.stem, bool(shape.flags & WOBBLE)
    own = [(i, j) for i in range(n - k + 1) for j in range(i, n - k + 1) if self_stem(g, i, j, k, shape.min_loop, w)]
    scaf = [(i, j) for i in range(n - k + 1) for j in range(len(s) - k + 1) if scaffold_stem(g, s, i, j, k, w)]
    return own, scaf


def longest(g, s, shape):
    """(self_longest, scaf_longest): the largest L with a stem, 0 when none.  A stem (i, j, L + 1) holds the stem (i + 1, j, L),
    so the lengths with a stem are 1 .. longest and the search stops at the first length without one."""
    n, w = len(g), bool(shape.flags & WOBBLE)
    own = scaf = 0
    while any(self_stem(g, i, j, own + 1, shape.min_loop, w) for i in range(n) for j in range(i, n)):
        own += 1
    while any(scaffold_stem(g, s, i, j, scaf + 1, w) for i in range(n) for j in range(len(s))):
        scaf += 1
    return own, scaf


_rows = {}


def fields(g, s, shape):
    """The six fields of spacer g against scaffold s as a dict."""
    g, s = letters(g), letters(s)
    key = (g, s, shape)
    if key in _rows:
        return _rows[key]
    assert len(g) == shape.proto_len
    k = shape.stem
    own, scaf = stems(g, s, shape)
    self5 = {i for i, _ in own if qual(g, i, shape)}
    scaf5 = {i for i, _ in scaf if qual(g, i, shape)}
    covered = set()
    for i, j in own:
        if qual(g, i, shape):
            covered |= set(range(i, i + k)) | set(range(j, j + k))
    for i in scaf5:
        covered |= set(range(i, i + k))
    seed = set(range(shape.seed_start, shape.seed_start + shape.seed_len))
    lo, ls = longest(g, s, shape)
    out = {"starts": len(self5 | scaf5), "self_starts": len(self5), "scaf_starts": len(scaf5), "seed_paired": len(covered & seed),
           "self_longest": lo, "scaf_longest": ls}
    _rows[key] = out
    return out


def row(g, s, shape):
    """ROW: (w0, w1) of a spacer text; a letter other than A C G T U gives the undefined row."""
    if any(ch not in "ACGT" for ch in letters(g)):
        return UNDEF, UNDEF
    f = fields(g, s, shape)
    return (f["starts"] | f["self_starts"] << 8 | f["scaf_starts"] << 16 | f["seed_paired"] << 24, f["self_longest"] | f["scaf_longest"] << 8)


def keep(r, limits):
    """FILTER for a row (w0, w1) and limits (max_starts, max_self_longest, max_scaf_longest, max_seed_paired)."""
    w0, w1 = int(r[0]), int(r[1])
    if w0 == UNDEF and w1 == UNDEF:
        return False
    values = (w0 & 0xFF, w1 & 0xFF, (w1 >> 8) & 0xFF, w0 >> 24)
    return all(v <= lim for v, lim in zip(values, limits))


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
SPCAS9 = Shape(23, 0, 20, 4, 2, 3, 8, 12, 0)
CAS12A = Shape(27, 4, 23, 4, 2, 3, 0, 6, 0)
# (name, shape, scaffold lengths): together every bound of SHAPE that a mask can get wrong, and every scaffold length at which
# the windows change their word
SHAPES = (
    ("SpCas9", SPCAS9, (0, 3, 4, 76)),
    ("Cas12a", CAS12A, (0, 20, 33)),
    ("SpCas9_wobble", SPCAS9._replace(flags=WOBBLE), (31, 64)),
    ("n12_site16", Shape(16, 2, 12, 3, 1, 0, 0, 4, 0), (0, 2, 3, 32)),            # the smallest spacer, k = 3 (k - 1 = 2, k = 3), min_loop 0
    ("n32_site32", Shape(32, 0, 32, 8, 4, 16, 16, 16, 0), (7, 8, 128)),           # bit 31 in play, k = 8, min_loop 16, seed at the 3' end
    ("n32_wobble", Shape(32, 0, 32, 5, 0, 0, 0, 16, WOBBLE), (65, 97)),           # gc_min 0, min_loop 0, seed at the 5' end
    ("at_site_end", Shape(30, 6, 24, 4, 4, 4, 12, 12, 0), (96,)),                 # proto_start + n = site_len, gc_min = k, seed at the 3' end
    ("no_seed", Shape(23, 1, 21, 6, 3, 5, 0, 0, WOBBLE), (0, 5, 6, 33)),          # seed_len 0
    ("seed_5prime", Shape(27, 4, 23, 3, 0, 2, 0, 16, 0), (31, 65)),               # k = 3 and gc_min 0
)
SHAPE_OF = {name: shape for name, shape, _ in SHAPES}


@functools.lru_cache(maxsize=None)
def scaffold(name, m):
    """The scaffold text of m letters for shape `name`, seeded; U and lower case among its letters."""
    rng = np.random.default_rng([35, m, len(name)])
    text = random_seq(rng, m)
    return "".join(("u" if ch == "T" else ch.lower()) if (i % 3 == 0) else ch for i, ch in enumerate(text))


def plant(n, pieces, background="A"):
    t = [background] * n
    for at, text in pieces:
        assert 0 <= at and at + len(text) <= n, (at, text, n)
        t[at:at + len(text)] = text
    return "".join(t)


def gc_word(rng, k, alphabet="GC"):
    return "".join(alphabet[int(b)] for b in rng.integers(0, len(alphabet), size=k))


@functools.lru_cache(maxsize=None)
def cases(name, m):
    """[(family, spacer)] for shape `name` against scaffold(name, m), seeded.  A family that does not fit the shape is left out."""
    shape = SHAPE_OF[name]
    n, k, loop = shape.proto_len, shape.stem, shape.min_loop
    s = letters(scaffold(name, m))
    rng = np.random.default_rng([35, 1, m, len(name)])
    out = []
    for _ in range(8):
        out.append(("random", random_seq(rng, n)))
    out.append(("none", "A" * n))
    for _ in range(2):
        out.append(("none", gc_word(rng, n, "AC")))  # no letter has its partner
    # hairpins in a background that pairs with nothing: the loop exactly min_loop, one shorter, the arms at both ends, longer arms
    for _ in range(2):
        arm = gc_word(rng, k)
        if 2 * k + loop <= n:
            i = int(rng.integers(0, n - 2 * k - loop + 1))
            out.append(("loop_exact", plant(n, [(i, arm), (i + k + loop, revcomp(arm))])))
            out.append(("end_to_end", plant(n, [(0, arm), (n - k, revcomp(arm))])))
        if loop >= 1 and 2 * k + loop - 1 <= n:
            i = int(rng.integers(0, n - 2 * k - loop + 2))
            out.append(("loop_short", plant(n, [(i, arm), (i + k + loop - 1, revcomp(arm))])))
        if 2 * (k + 2) + loop <= n:
            arm2 = gc_word(rng, k + 2)
            i = int(rng.integers(0, n - 2 * (k + 2) - loop + 1))
            out.append(("long_self", plant(n, [(i, arm2), (n - k - 2, revcomp(arm2))])))
    if 2 * k + loop <= n:
        for arm in ("G" * k, ("GGC" * 3)[:k], ("TGC" * 3)[:k]):  # the partner that pairs under WOBBLE alone where there is one
            partner = "".join({"G": "T", "C": "G", "A": "T", "T": "G"}[a] for a in reversed(arm))
            out.append(("wobble_only", plant(n, [(0, arm), (n - k, partner)], "C")))
        at_arm = gc_word(rng, k, "AT")
        out.append(("unqualified", plant(n, [(0, at_arm), (n - k, revcomp(at_arm))], "C")))  # no G/C in the 5' arm
    if n % 2 == 0:
        half = random_seq(rng, n // 2)
        out.append(("palindrome", half + revcomp(half)))
        out.append(("palindrome", ("GC" * n)[:n]))
    # scaffold stems: the spacer carries the reverse complement of a scaffold word
    if m >= k:
        at = {0, m - k}
        for b in (32, 64, 96):
            if k // 2 <= b and b - k // 2 + k <= m:
                at.add(b - k // 2)
        for j in sorted(at):
            for i in sorted({0, n - k, int(rng.integers(0, n - k + 1))}):
                out.append(("scaffold", plant(n, [(i, revcomp(s[j:j + k]))], "A" if (i + j) % 2 else "C")))
        width = min(m, n - shape.seed_start, max(shape.seed_len, k) + 2)
        j = int(rng.integers(0, m - width + 1))
        if width >= k:
            out.append(("seed_full", plant(n, [(shape.seed_start, revcomp(s[j:j + width]))])))
        width = min(m, n)
        j = int(rng.integers(0, m - width + 1))
        out.append(("scaffold_long", plant(n, [(n - width, revcomp(s[j:j + width]))])))
        arm = gc_word(rng, k)
        if 3 * k + loop <= n:
            out.append(("both", plant(n, [(0, arm), (k + loop, revcomp(arm)), (n - k, revcomp(s[m - k:m]))])))
    return tuple(out)


def seen(name, m):
    """family -> the set of things its cases of (name, m) show, found on the strings alone."""
    shape = SHAPE_OF[name]
    s = letters(scaffold(name, m))
    k, loop, n = shape.stem, shape.min_loop, shape.proto_len
    plain = shape._replace(flags=0)
    out = collections.defaultdict(set)
    for family, g in cases(name, m):
        f = fields(g, s, shape)
        own, scaf = stems(g, s, shape)
        tags = out[family]
        tags.add("starts == 0" if f["starts"] == 0 else "starts > 0")
        if f["self_starts"] and not f["scaf_starts"]:
            tags.add("self only")
        if f["scaf_starts"] and not f["self_starts"]:
            tags.add("scaffold only")
        if f["scaf_starts"] and f["self_starts"]:
            tags.add("both")
        if any(j - (i + k) == loop and qual(g, i, shape) for i, j in own):
            tags.add("loop == min_loop")
        if loop and not own and any(self_stem(g, i, i + k + loop - 1, k, loop - 1, bool(shape.flags & WOBBLE)) for i in range(n)):
            tags.add("loop == min_loop - 1 does not count")
        if (0, n - k) in own:
            tags.add("position 0 with n - 1")
        if f["self_longest"] >= k + 2:
            tags.add("self_longest >= k + 2")
        if shape.flags & WOBBLE and set(own) - set(stems(g, s, plain)[0]):
            tags.add("only under WOBBLE")
        if shape.gc_min and f["self_longest"] >= k and any(not qual(g, i, shape) for i, _ in own) and not f["self_starts"]:
            tags.add("fails QUAL, lengthens self_longest")
        for i, j in scaf:
            if qual(g, i, shape):
                if j == 0:
                    tags.add("scaffold position 0")
                if j == len(s) - k:
                    tags.add("scaffold position m - k")
                for b in (32, 64, 96):
                    if j < b < j + k:
                        tags.add("across %d" % b)
        if f["seed_paired"] == 0:
            tags.add("seed_paired == 0")
        if shape.seed_len and f["seed_paired"] == shape.seed_len:
            tags.add("seed_paired == seed_len")
        if g == revcomp(g):
            tags.add("palindromic")
    return out


# ---- the small genome ------------------------------------------------------------------------------------------------------------
def offsets(contigs):
    """Global position of every contig's first base: the contigs lie one N apart (PackedGenome.from_sequences)."""
    off, at = [], 0
    for s in contigs:
        off.append(at)
        at += len(s) + 1
    return off


def site_of(rng, spacer, shape):
    """A site of site_len letters that carries the spacer where the shape reads it."""
    return random_seq(rng, shape.proto_start) + spacer + random_seq(rng, shape.site_len - shape.proto_start - shape.proto_len)


@functools.lru_cache(maxsize=None)
def small_genome(name, m):
    """A few hundred bases: contigs of site_len - 1, site_len and site_len + 1 bases, then a long one that carries the sites of
    half the planted cases of (name, m) on '+' and the other half on '-', with an N run between two of them, then one of 70
    random bases.  The one-N separators and the word boundaries at 32, 64, ... fall inside sites."""
    shape = SHAPE_OF[name]
    rng = np.random.default_rng([35, 2, m, len(name)])
    L = shape.site_len
    seqs = [random_seq(rng, n) for n in (L - 1, L, L + 1)]
    main = random_seq(rng, 5)
    by_family = collections.OrderedDict()
    for family, g in cases(name, m):
        if family != "random":
            by_family.setdefault(family, []).append(g)
    planted = [g for k in range(3) for gs in by_family.values() for g in gs[k:k + 1]]  # every family first, then their second cases
    for i, g in enumerate(planted[:16 if shape.proto_len < 32 else 12]):  # (the restatement is cubic in the spacer)
        site = site_of(rng, g, shape)
        main += (revcomp(site) if i % 2 else site) + random_seq(rng, int(rng.integers(0, 3)))
        if i == 4:
            main += "NN"
    seqs.append(main)
    seqs.append(random_seq(rng, 70))
    return tuple(seqs)


def every_locus(contigs):
    """Every (contig, p, strand) with p in [0, len]: the last site_len starts of a contig name a site that leaves it."""
    return [(c, p, s) for c, text in enumerate(contigs) for p in range(len(text) + 1) for s in (0, 1)]


def locus_array(loci):
    out = np.zeros(len(loci), dtype=va.LOCUS_DTYPE)
    if len(loci):
        a = np.asarray(loci, dtype=np.int64).reshape(-1, 3)
        out["contig"], out["pos"], out["strand"] = a[:, 0] & 0xFFFFFFFF, a[:, 1] & 0xFFFFFFFF, a[:, 2] & 0xFFFFFFFF
    return out


def classify(contigs, locus, shape, resident=None):
    """(class, spacer text or None) of locus (contig, pos, strand): SPACER and CLASS in their order.  resident: None (the whole
    genome is) or the half-open range of global positions the genome object holds."""
    c, p, strand = locus
    if c >= len(contigs) or strand > 1 or p + shape.site_len > len(contigs[c]):
        return "invalid", None
    if resident is not None:
        g = offsets(contigs)[c] + p
        if g < resident[0] or g + shape.site_len > resident[1]:
            return "not_resident", None
    text = contigs[c][p:p + shape.site_len].upper()
    if any(ch not in "ACGT" for ch in text):
        return "has_n", None
    site = revcomp(text) if strand else text
    return "defined", site[shape.proto_start:shape.proto_start + shape.proto_len]


def expected(contigs, loci, shape, scaffold_text, resident=None):
    """(uint32[n, 2] rows, stats dict, [spacer or None]) of loci under shape and scaffold."""
    out = np.empty((len(loci), 2), dtype=np.uint32)
    stats = dict.fromkeys(CLASSES, 0)
    texts = []
    for i, locus in enumerate(loci):
        cls, text = classify(contigs, locus, shape, resident)
        stats[cls] += 1
        texts.append(text)
        out[i] = row(text, scaffold_text, shape) if cls == "defined" else (UNDEF, UNDEF)
    return out, stats, texts

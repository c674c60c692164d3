"""Shared helpers of test_efficiency.py (GPU) and test_efficiency_cpu.py: the definition of the on-target efficiency score
(include/varscot_hip.h: SHAPE, CONTEXT, MODEL, LINEAR, UNDEF) in plain Python - the context by string slicing and reverse
complement, the sum with Python floats in the order of the definition, the classes in theirs - the seeded model families and the
small genomes of the tests.  Nothing here calls the library but `build`, which hands a family's arrays to va.EfficiencyModel."""
import functools
import math
import struct

import numpy as np

import varscot_amd as va
from helpers import random_seq, revcomp

SHAPES = [(4, 23, 3), (6, 23, 6), (0, 16, 0), (16, 32, 16), (0, 23, 16), (16, 23, 0)]  # (up, site_len, down); C = 64 among them
FAMILIES = ("dense", "sparse", "zero", "mixed")
UNDEF = va.EFF_UNDEFINED_BITS
CLASSES = ("defined", "invalid", "off_contig", "not_resident", "has_n")


def bits(x):
    """The 64 bits of a Python float."""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- models ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def arrays(family, shape, seed=0):
    """{"intercept", "mono" [C][4], "di" [C - 1][16], "gc", "gc_range"} of a seeded model of one family:
      dense   every weight a normal deviate, a G/C table over the first 20 (or site_len) bases of the site
      sparse  "Rule-Set-1-like": about 70 features that are not 0 and a piecewise-linear G/C table
      zero    nothing but zeros, no G/C term
      mixed   magnitudes of 1e16, 1 and 1e-16 side by side: another order of the additions gives other bits."""
    up, site_len, down = shape
    C = up + site_len + down
    rng = np.random.default_rng([seed, FAMILIES.index(family), up, site_len, down])
    mono, di = np.zeros((C, 4)), np.zeros((C - 1, 16))
    gc_range = (up, min(20, site_len))
    if family == "dense":
        mono, di = rng.normal(size=(C, 4)), rng.normal(size=(C - 1, 16))
        gc, intercept = rng.normal(size=gc_range[1] + 1), float(rng.normal())
    elif family == "sparse":
        for k in rng.choice(C * 4, size=min(30, C * 4), replace=False):
            mono[k // 4, k % 4] = rng.normal(scale=0.2)
        for k in rng.choice((C - 1) * 16, size=40, replace=False):
            di[k // 16, k % 16] = rng.normal(scale=0.2)
        mid = gc_range[1] // 2
        gc = np.array([-0.2026259 * (mid - k) if k < mid else -0.1665878 * (k - mid) for k in range(gc_range[1] + 1)]) + 0.0  # (-0.0 at mid -> +0.0)
        intercept = 0.59763615
    elif family == "zero":
        gc, gc_range, intercept = None, None, 0.0
    else:
        scale = np.array([1e16, 1.0, 1e-16])
        mono = rng.choice([-1.0, 1.0], size=(C, 4)) * scale[rng.integers(0, 3, size=(C, 4))] * rng.uniform(1, 2, size=(C, 4))
        di = rng.choice([-1.0, 1.0], size=(C - 1, 16)) * scale[rng.integers(0, 3, size=(C - 1, 16))] * rng.uniform(1, 2, size=(C - 1, 16))
        gc = rng.choice([-1.0, 1.0], size=gc_range[1] + 1) * scale[rng.integers(0, 3, size=gc_range[1] + 1)]
        intercept = 1.0
    for a in (mono, di) + (() if gc is None else (gc,)):
        a.setflags(write=False)
    return {"intercept": intercept, "mono": mono, "di": di, "gc": gc, "gc_range": gc_range}


def build(family, shape, seed=0, link="identity"):
    a = arrays(family, shape, seed)
    return va.EfficiencyModel(shape[0], shape[1], shape[2], a["intercept"], a["mono"], a["di"], gc=a["gc"], gc_range=a["gc_range"], link=link)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def py_linear(a, text):
    """LINEAR over a context in read orientation; a = arrays(..).  Python floats are IEEE doubles: every + rounds once."""
    b = ["ACGT".index(ch) for ch in text]
    mono, di = a["mono"], a["di"]
    x = float(a["intercept"])
    for j in range(len(b)):
        x = x + float(mono[j][b[j]])
    for j in range(len(b) - 1):
        x = x + float(di[j][4 * b[j] + b[j + 1]])
    if a["gc_range"] is not None and a["gc_range"][1]:
        s, n = a["gc_range"]
        x = x + float(a["gc"][sum(ch in "GC" for ch in text[s:s + n])])
    return x


def py_linear_bits(a, text):
    """... as its bits; the undefined NaN where the text holds a letter outside ACGT."""
    return UNDEF if any(ch not in "ACGT" for ch in text.upper()) else bits(py_linear(a, text.upper()))


def offsets(contigs):
    """Global position of every contig's first base: the contigs lie one N apart (PackedGenome.from_sequences)."""
    off, at = [], 0
    for s in contigs:
        off.append(at)
        at += len(s) + 1
    return off


def classify(contigs, locus, shape, resident=None):
    """(class, context text or None) of locus (contig, pos, strand): CONTEXT and UNDEF in their order.  resident: None (the
    whole genome is) or the half-open range of global positions the genome object holds."""
    up, site_len, down = shape
    c, p, strand = locus
    if c >= len(contigs) or strand > 1 or p + site_len > len(contigs[c]):
        return "invalid", None
    left, right = (down, up) if strand else (up, down)
    if p - left < 0 or p + site_len + right > len(contigs[c]):
        return "off_contig", None
    if resident is not None:
        g = offsets(contigs)[c] + p - left
        if g < resident[0] or g + up + site_len + down > resident[1]:
            return "not_resident", None
    text = contigs[c][p - left:p + site_len + right].upper()
    if any(ch not in "ACGT" for ch in text):
        return "has_n", None
    return "defined", revcomp(text) if strand else text


def expected(contigs, loci, shape, a, resident=None):
    """(uint64 bits of the predictors, stats dict) of loci [(contig, pos, strand)] under model arrays a."""
    out = np.empty(len(loci), dtype=np.uint64)
    stats = dict.fromkeys(CLASSES, 0)
    memo = {}
    for i, locus in enumerate(loci):
        if locus not in memo:
            cls, text = classify(contigs, locus, shape, resident)
            memo[locus] = (cls, bits(py_linear(a, text)) if cls == "defined" else UNDEF)
        cls, b = memo[locus]
        stats[cls] += 1
        out[i] = b
    return out, stats


def py_logistic(x):
    return 1.0 / (1.0 + math.exp(-x))


# ---- genomes -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_genome(shape):
    """Contigs of C - 1, C and C + 1 bases, 5 bases, 200 bases with one N at 100, and 131 bases: about 500 bases whose one-N
    separators and word boundaries at 32, 64, ... fall inside contexts."""
    C = sum(shape)
    rng = np.random.default_rng([11, C, shape[0]])
    seqs = [random_seq(rng, n) for n in (C - 1, C, C + 1, 5, 200, 131)]
    seqs[4] = seqs[4][:100] + "N" + seqs[4][101:]
    return tuple(seqs)


def every_locus(contigs, site_len):
    """Every (contig, p, strand) with p in [0, len - site_len]."""
    return [(c, p, s) for c, text in enumerate(contigs) for p in range(len(text) - site_len + 1) for s in (0, 1)]


def locus_array(loci):
    out = np.zeros(len(loci), dtype=va.LOCUS_DTYPE)
    if len(loci):
        a = np.asarray(loci, dtype=np.int64).reshape(-1, 3)
        out["contig"], out["pos"], out["strand"] = a[:, 0] & 0xFFFFFFFF, a[:, 1] & 0xFFFFFFFF, a[:, 2] & 0xFFFFFFFF
    return out

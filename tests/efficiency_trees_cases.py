"""Shared helpers of test_efficiency_trees.py (GPU) and test_efficiency_trees_cpu.py: the definition of the tree-ensemble
efficiency score (include/varscot_hip.h: SUMS, TREES, PREDICTOR) in plain Python - the sums with Python ints over the letters
of the context, the walk over the node tuples as the caller writes them, the leaves added as Python floats in tree order - and
the seeded model families.  The context, its classes and the small genomes are efficiency_cases' (the definition shares them).
Nothing here calls the library but `build`, which hands a family's lists to va.TreeEfficiencyModel."""
import functools

import numpy as np

import varscot_amd as va
from efficiency_cases import SHAPES, UNDEF, CLASSES, bits, classify  # noqa: F401  (re-exported for the tests)

FAMILIES = ("azimuth", "stumps", "chain", "leaf1", "leaf1024", "mixed", "largest", "edges")
LETTERS = "ACGT"
DINUCS = [x + y for x in LETTERS for y in LETTERS]


# ---- the definition ----------------------------------------------------------------------------------------------------------
def py_sum(s, text):
    """S_i of a context: s = (start, length, {letters: weight})."""
    start, length, wts = s
    part = text[start:start + length]
    total = 0
    for j, ch in enumerate(part):
        total += wts.get(ch, 0)
        if j + 1 < len(part):
            total += wts.get(part[j:j + 2], 0)
    return total


def py_test(node, text, S):
    kind = node[0]
    if kind == "base":
        return text[node[1]] in node[2]
    if kind == "pair":
        pairs = node[3].split(",") if isinstance(node[3], str) else node[3]
        return text[node[1]] + text[node[2]] in pairs
    return S[node[1]] <= node[2]


def py_predict(model, text):
    """PREDICTOR over a context in read orientation; model = {"base", "sums", "trees"}.  Python floats: every + rounds once."""
    S = [py_sum(s, text) for s in model["sums"]]
    x = float(model["base"])
    for tree in model["trees"]:
        k = 0
        while tree[k][0] != "leaf":
            k = tree[k][-2] if py_test(tree[k], text, S) else tree[k][-1]
        x = x + float(tree[k][1])
    return x


def py_predict_bits(model, text):
    return UNDEF if any(ch not in LETTERS for ch in text.upper()) else bits(py_predict(model, text.upper()))


def path_lengths(model, text):
    """Nodes visited per tree (the leaf included) - what the chain family is about."""
    S = [py_sum(s, text) for s in model["sums"]]
    out = []
    for tree in model["trees"]:
        k, n = 0, 1
        while tree[k][0] != "leaf":
            k = tree[k][-2] if py_test(tree[k], text, S) else tree[k][-1]
            n += 1
        out.append(n)
    return out


def expected(contigs, loci, shape, model, resident=None):
    """(uint64 bits of the predictors, stats dict) of loci [(contig, pos, strand)] under a model."""
    out = np.empty(len(loci), dtype=np.uint64)
    stats = dict.fromkeys(CLASSES, 0)
    memo, by_text = {}, {}
    for i, locus in enumerate(loci):
        if locus not in memo:
            cls, text = classify(contigs, locus, shape, resident)
            if cls == "defined" and text not in by_text:
                by_text[text] = bits(py_predict(model, text))
            memo[locus] = (cls, by_text[text] if cls == "defined" else UNDEF)
        cls, b = memo[locus]
        stats[cls] += 1
        out[i] = b
    return out, stats


# ---- models ------------------------------------------------------------------------------------------------------------------
def _number(nested, order):
    """A nested tree - ("leaf", v) or (test..., left subtree, right subtree) - as a node list numbered in preorder ("pre") or
    level by level ("level"): either way a child's number is larger than its parent's."""
    seq, queue = [], [nested]
    while queue:
        n = queue.pop(0 if order == "level" else -1)
        seq.append(n)
        if n[0] != "leaf":
            queue += [n[-2], n[-1]] if order == "level" else [n[-1], n[-2]]
    at = {id(n): k for k, n in enumerate(seq)}
    return [n if n[0] == "leaf" else n[:-2] + (at[id(n[-2])], at[id(n[-1])]) for n in seq]


def _random_test(rng, C, sums, kinds):
    kind = kinds[int(rng.integers(len(kinds)))]
    if kind == "sum" and not sums:
        kind = "base"
    if kind == "base":
        return ("base", int(rng.integers(C)), "".join(ch for ch in LETTERS if rng.random() < 0.4))
    if kind == "pair":
        a = int(rng.integers(C))
        b = int(rng.integers(C - 1))
        b += b >= a
        if rng.random() < 0.5:  # the position-specific dinucleotide, as Rule Set 2 has it
            a = int(rng.integers(C - 1))
            b = a + 1
        return ("pair", a, b, [d for d in DINUCS if rng.random() < 0.3])
    i = int(rng.integers(len(sums)))
    text = "".join(LETTERS[k] for k in rng.integers(0, 4, C))  # a threshold on or next to a sum some context has
    return ("sum", i, py_sum(sums[i], text) + int(rng.integers(-1, 2)))


def _random_tree(rng, depth, C, sums, leaf, kinds=("base", "pair", "sum")):
    if depth == 0:
        return ("leaf", leaf(rng))
    return _random_test(rng, C, sums, kinds) + (_random_tree(rng, depth - 1, C, sums, leaf, kinds), _random_tree(rng, depth - 1, C, sums, leaf, kinds))


def _three_sums(rng, shape):
    up, site_len, down = shape
    C = sum(shape)
    di = {d: int(w) for d, w in zip(DINUCS, rng.integers(-300, 100, 16))}  # a nearest-neighbour-like table, mostly negative
    di["GG"] = 0
    return [(up, min(20, site_len), {"G": 1, "C": 1}), (0, C, {"T": 1}), (up, site_len, di)]


@functools.lru_cache(maxsize=None)
def lists(family, shape, seed=0):
    """{"base", "sums", "trees"} of a seeded model of one family:
      azimuth   100 trees of depth 3, the four kinds mixed, 3 sums: G/C of the protospacer, a letter's count, weighted dinucleotides
      stumps    64 trees of one test and two leaves
      chain     a chain of depth 32 (tree 31) beside 63 single-leaf trees: one lane walks far longer than its neighbours
      leaf1     one single-leaf tree;  leaf1024: 1 024 of them
      mixed     leaves of 1e16, 1 and 1e-16 side by side, numbered level by level: another order of the additions gives other bits
      largest   8 192 nodes in 546 trees, 16 sums
      edges     thresholds on and one below attainable sums, masks 0 and all-ones, a PAIR with pos_a > pos_b, positions 0 and
                C - 1, ranges of length 0, 1 and C"""
    up, site_len, down = shape
    C = sum(shape)
    rng = np.random.default_rng([seed, FAMILIES.index(family), up, site_len, down])
    normal = lambda r: float(r.normal(scale=0.05))  # noqa: E731
    sums, base = [], 0.0
    if family == "azimuth":
        sums, base = _three_sums(rng, shape), 0.4921
        trees = [_number(_random_tree(rng, 3, C, sums, normal), "pre") for _ in range(100)]
    elif family == "stumps":
        sums = _three_sums(rng, shape)
        trees = [_number(_random_tree(rng, 1, C, sums, normal), "pre") for _ in range(64)]
    elif family == "chain":
        sums, base = _three_sums(rng, shape), -1.0
        nested = ("leaf", normal(rng))
        for k in range(32):  # every inner node: one leaf, one deeper node.  Every fourth test lets three letters of four go
            # deeper, the others are constant (on a side that changes): a tenth of the contexts walk all 32 edges
            pos = int(rng.integers(C))
            if k % 4 == 0:
                test, deeper_left = ("base", pos, "".join(rng.permutation(list(LETTERS))[:3])), True
            else:
                test, deeper_left = [(("base", pos, "ACGT"), True), (("pair", pos, (pos + 1) % C, []), False), (("sum", 1, C), True),
                                     (("sum", 0, -1), False)][int(rng.integers(4))]
            nested = test + ((nested, ("leaf", normal(rng))) if deeper_left else (("leaf", normal(rng)), nested))
        trees = [[("leaf", normal(rng))] for _ in range(64)]
        trees[31] = _number(nested, "pre")
    elif family in ("leaf1", "leaf1024"):
        base = 0.1
        trees = [[("leaf", float(rng.normal()))] for _ in range(1 if family == "leaf1" else 1024)]
    elif family == "mixed":
        sums, base = _three_sums(rng, shape), 1.0
        big = lambda r: float(r.choice([-1.0, 1.0]) * [1e16, 1.0, 1e-16][int(r.integers(3))] * r.uniform(1, 2))  # noqa: E731
        trees = [_number(_random_tree(rng, 2, C, sums, big), "level") for _ in range(60)]
    elif family == "largest":
        for i in range(16):
            start = int(rng.integers(0, C))
            length = int(rng.integers(0, C - start + 1))
            wts = {LETTERS[int(k)]: int(rng.integers(-2 ** 20, 2 ** 20 + 1)) for k in rng.choice(4, size=2, replace=False)}
            wts.update({DINUCS[int(k)]: int(rng.integers(-2 ** 20, 2 ** 20 + 1)) for k in rng.choice(16, size=i % 5, replace=False)})
            sums.append((start, length, wts))
        sums[0] = (0, C, dict({ch: 2 ** 20 for ch in LETTERS}, **{d: 2 ** 20 for d in DINUCS}))  # the largest sum there is
        sums[1] = (0, C, dict({ch: -2 ** 20 for ch in LETTERS}, **{d: -2 ** 20 for d in DINUCS}))
        trees = [_number(_random_tree(rng, 3, C, sums, normal), "pre" if t % 2 else "level") for t in range(544)]
        trees += [_number(_random_tree(rng, 4, C, sums, normal), "level"), [("leaf", normal(rng))]]
        assert sum(len(t) for t in trees) == 8192
    else:
        gc_len = min(20, site_len)
        sums = [(up, gc_len, {"G": 1, "C": 1}), (C // 2, 0, {"A": 5, "AA": 7}), (C - 1, 1, {"A": 1, "C": 2, "G": 3, "T": 4, "AA": 100}),
                (0, C, {"A": -3, "AC": 11, "TT": -2 ** 20, "G": 2 ** 20}), (C, 0, {"T": 1})]
        leaf = iter(float(v) for v in rng.normal(size=4000))
        stump = lambda *test: [test + (1, 2), ("leaf", next(leaf)), ("leaf", next(leaf))]  # noqa: E731
        trees = [stump("sum", 0, t) for t in range(-1, gc_len + 2)]                      # every attainable G/C count, one below, one above
        trees += [stump("sum", 1, t) for t in (-1, 0, 1)] + [stump("sum", 4, t) for t in (-1, 0)]  # a range of length 0: S = 0
        trees += [stump("sum", 2, t) for t in range(0, 6)]                               # a range of length 1: no dinucleotide fits
        trees += [stump("sum", 3, t) for t in (-2 ** 31, -2 ** 27, -2 ** 20 - 1, -2 ** 20, -3 * C, -3 * C - 1, 0, 2 ** 20, 2 ** 27 - 1, 2 ** 27, 2 ** 31 - 1)]
        for pos in (0, C - 1, up):
            trees += [stump("base", pos, m) for m in ("", "ACGT", "A", "CGT", "T", "G")]
        trees += [stump("pair", C - 1, 0, ["AC"]), stump("pair", 0, C - 1, ["AC"]), stump("pair", C - 1, 0, ["CA", "GT", "TT"]),
                  stump("pair", 0, C - 1, []), stump("pair", C - 1, 0, list(DINUCS)), stump("pair", 5, 4, ["AC", "AG", "AT"]),
                  stump("pair", up + 3, up, ["GT"]), stump("pair", 1, 0, ["TG"])]
    model = {"base": base, "sums": tuple((s, n, dict(w)) for s, n, w in sums), "trees": tuple(tuple(t) for t in trees)}
    return model


def build(family, shape, seed=0, link="identity"):
    m = lists(family, shape, seed)
    return va.TreeEfficiencyModel(shape[0], shape[1], shape[2], m["base"], m["sums"], m["trees"], link=link)

"""The host side of the tree-ensemble efficiency score (include/varscot_hip.h "regression-tree ensembles"), without a device:
vsc_eff_trees_score_text - the functions the kernels run - against the Python restatement to the bit, every refusal of
vsc_eff_trees_build on its own, the -0.0 normalisation, the link, the model file, two cross-checks against the linear model
and the conversion of a scikit-learn GradientBoostingRegressor."""
import ctypes as C
import math

import numpy as np
import pytest

import efficiency_cases as ec
import efficiency_trees_cases as tc
import varscot_amd as va
from helpers import random_seq
from varscot_amd import _lib


def _texts(C_, n=25, seed=7):
    rng = np.random.default_rng(seed)
    return [random_seq(rng, C_) for _ in range(n)] + ["A" * C_, "C" * C_, "G" * C_, "T" * C_, ("ACGT" * 16)[:C_], ("GGCC" * 16)[:C_]]


@pytest.mark.parametrize("shape", tc.SHAPES, ids=lambda s: "%d-%d-%d" % s)
@pytest.mark.parametrize("family", tc.FAMILIES)
def test_score_text_equals_the_restatement(family, shape):
    model = tc.lists(family, shape)
    m = tc.build(family, shape)
    C_ = sum(shape)
    texts = _texts(C_, n=6 if family == "largest" else 25)
    texts.append(texts[0].lower())
    for t in texts:
        assert tc.bits(m.score_text(t)) == tc.py_predict_bits(model, t), t
    for at in (0, C_ // 2, C_ - 1):  # a letter outside ACGT, anywhere: undefined, the one NaN
        t = texts[1][:at] + "N" + texts[1][at + 1:]
        assert tc.bits(m.score_text(t)) == tc.UNDEF
    for t in (texts[0][:-1], texts[0] + "A", ""):  # another length is refused
        with pytest.raises(va.VarscotError) as e:
            m.score_text(t)
        assert e.value.code == -22
    info = m.info()
    assert (info["up"], info["site_len"], info["down"], info["link"]) == shape + ("identity",)
    kinds = [n[0] for t in model["trees"] for n in t]
    assert info["n_sums"] == len(model["sums"]) and info["n_trees"] == len(model["trees"]) and info["n_nodes"] == len(kinds)
    assert [info[k] for k in ("leaves", "base_nodes", "pair_nodes", "sum_nodes")] == [kinds.count(k) for k in ("leaf", "base", "pair", "sum")]
    depth = {"azimuth": 3, "stumps": 1, "chain": 32, "leaf1": 0, "leaf1024": 0, "mixed": 2, "largest": 4, "edges": 1}[family]
    assert info["max_depth"] == depth


def test_the_families_are_what_they_claim():
    shape = (4, 23, 3)
    assert sum(len(t) for t in tc.lists("largest", shape)["trees"]) == 8192 and len(tc.lists("largest", shape)["sums"]) == 16
    assert len(tc.lists("leaf1024", shape)["trees"]) == 1024
    chain = tc.lists("chain", shape)
    walks = [max(tc.path_lengths(chain, t)) for t in _texts(30, n=300)]
    assert max(walks) == 33 and min(walks) <= 5 and sorted(len(t) for t in chain["trees"])[-2:] == [1, 65]  # some walk all 32 edges, some stop early
    # the mixed family exists so that a reassociated sum is caught: adding the leaves in reverse gives other bits somewhere
    mixed = tc.lists("mixed", shape)
    rev = dict(mixed, trees=mixed["trees"][::-1])
    assert any(tc.py_predict_bits(mixed, t) != tc.py_predict_bits(rev, t) for t in _texts(30))
    # the edges family separates <= from <: with < in the SUM test some context scores otherwise
    edges = tc.lists("edges", shape)
    strict = dict(edges, trees=tuple(tuple((n[0], n[1], n[2] - 1) + n[3:] if n[0] == "sum" else n for n in t) for t in edges["trees"]))
    assert any(tc.py_predict_bits(edges, t) != tc.py_predict_bits(strict, t) for t in _texts(30))
    # ... and the PAIR index is 4 b_a + b_b: with the letters swapped some context scores otherwise
    swapped = dict(edges, trees=tuple(tuple(n[:3] + ([p[::-1] for p in n[3]],) + n[4:] if n[0] == "pair" else n for n in t) for t in edges["trees"]))
    assert any(tc.py_predict_bits(edges, t) != tc.py_predict_bits(swapped, t) for t in _texts(30, n=200))


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _node(kind, a=0, b=0, mask=0, t=0, left=0, right=0, value=0.0, reserved=0):
    return (kind, a, b, mask, t, left, right, reserved, value)


LEAF = _node(0, value=1.0)


def _build(trees, sums=(), shape=None, base=0.0, n_trees=None, first=None):
    """The return code of vsc_eff_trees_build for raw nodes: trees = lists of _node tuples."""
    shape = shape or _lib.EffShape(4, 23, 3, 0, 0, 0)
    nodes = np.array([n for t in trees for n in t], dtype=_lib.EFF_NODE_DTYPE)
    if first is None:
        first = np.concatenate([[0], np.cumsum([len(t) for t in trees])])
    first = np.asarray(first, dtype=np.uint32)
    sum_arr = np.zeros(len(sums), dtype=_lib.EFF_SUM_DTYPE)
    for i, (start, length, mono, di) in enumerate(sums):
        sum_arr[i] = (start, length, mono, di)
    h = C.c_void_p()
    code = va.lib().vsc_eff_trees_build(C.byref(shape), float(base), _lib.ptr(sum_arr) if len(sums) else None, len(sums), _lib.ptr(nodes),
                                        _lib.ptr(first), len(trees) if n_trees is None else n_trees, C.byref(h))
    if code == 0:
        va.lib().vsc_eff_trees_free(h)
    else:
        assert not h.value
    return code


def _chain(depth):
    """A tree that is a chain of `depth` edges: node 2 k is inner with the leaf 2 k + 1 and the next inner node 2 k + 2."""
    nodes = []
    for k in range(depth):
        nodes += [_node(1, a=k % 30, mask=5, left=2 * k + 1, right=2 * k + 2), LEAF]
    return nodes + [LEAF]


ZERO_SUM = (0, 30, [0] * 4, [0] * 16)
STUMP = [_node(1, a=3, mask=5, left=1, right=2), LEAF, LEAF]
REFUSALS = {
    "child not larger than its parent": [[_node(1, a=3, mask=5, left=1, right=2), _node(1, a=4, mask=1, left=1, right=3), LEAF, LEAF]],
    "child equal to the root": [[_node(1, a=3, mask=5, left=0, right=1), LEAF]],
    "child outside the tree": [[_node(1, a=3, mask=5, left=1, right=3), LEAF, LEAF]],
    "child in the next tree": [[_node(1, a=3, mask=5, left=1, right=2), LEAF], [LEAF]],
    "node with two parents": [[_node(1, a=3, mask=5, left=1, right=2), _node(1, a=4, mask=1, left=2, right=3), LEAF, LEAF]],
    "both children the same node": [[_node(1, a=3, mask=5, left=1, right=1), LEAF]],
    "node with no parent": [[_node(1, a=3, mask=5, left=1, right=2), LEAF, LEAF, LEAF]],
    "depth of 33": [_chain(33)],
    "8 193 nodes": [_chain(32)] * 126 + [[LEAF]] * 3,
    "value that is not finite": [[_node(0, value=math.inf)]],
    "value that is NaN": [STUMP[:2] + [_node(0, value=math.nan)]],
    "pos_a == pos_b": [[_node(2, a=7, b=7, mask=1, left=1, right=2), LEAF, LEAF]],
    "position outside the context": [[_node(1, a=30, mask=1, left=1, right=2), LEAF, LEAF]],
    "pair position outside the context": [[_node(2, a=0, b=30, mask=1, left=1, right=2), LEAF, LEAF]],
    "mask wider than four bits": [[_node(1, a=0, mask=16, left=1, right=2), LEAF, LEAF]],
    "mask wider than sixteen bits": [[_node(2, a=0, b=1, mask=1 << 16, left=1, right=2), LEAF, LEAF]],
    "sum that does not exist": [[_node(3, a=0, t=1, left=1, right=2), LEAF, LEAF]],
    "unknown kind": [[_node(4, a=0, left=1, right=2), LEAF, LEAF]],
    "reserved field": [[_node(0, value=1.0, reserved=1)]],
    "leaf with children": [[_node(0, value=1.0, left=1, right=2), LEAF, LEAF]],
}


def test_accepted_models_next_to_the_refusals():
    assert _build([STUMP]) == 0
    assert _build([_chain(32)]) == 0                                           # depth 32
    assert _build([_chain(32)] * 126 + [[LEAF]] * 2) == 0                      # 8 192 nodes
    assert _build([[LEAF]] * 1024) == 0                                        # 1 024 trees
    assert _build([[_node(3, a=0, t=1, left=1, right=2), LEAF, LEAF]], sums=[ZERO_SUM]) == 0
    assert _build([STUMP], sums=[(0, 30, [2 ** 20, -2 ** 20, 0, 0], [2 ** 20] + [0] * 15)]) == 0
    assert _build([STUMP], sums=[(30, 0, [1] * 4, [0] * 16), (0, 0, [1] * 4, [0] * 16), (29, 1, [1] * 4, [0] * 16)]) == 0
    assert _build([STUMP], sums=[ZERO_SUM] * 16) == 0
    assert _build([[_node(2, a=29, b=0, mask=0xFFFF, left=2, right=1), LEAF, LEAF]]) == 0  # the children in either order


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_build_refuses_a_tree(what):
    assert _build(REFUSALS[what]) == -22, what


@pytest.mark.parametrize("what,sums", [
    ("weight of 2^20 + 1", [(0, 30, [2 ** 20 + 1, 0, 0, 0], [0] * 16)]),
    ("weight of -(2^20 + 1)", [(0, 30, [0] * 4, [0] * 15 + [-2 ** 20 - 1])]),
    ("range that leaves the context", [(11, 20, [1] * 4, [0] * 16)]),
    ("range that starts behind the context", [(31, 0, [1] * 4, [0] * 16)]),
    ("range that wraps around", [(0xFFFFFFF0, 0x20, [1] * 4, [0] * 16)]),
    ("17 sums", [ZERO_SUM] * 17),
])
def test_build_refuses_a_sum(what, sums):
    assert _build([STUMP], sums=sums) == -22, what


def test_build_refuses_shapes_counts_and_nulls():
    ok = lambda **k: _lib.EffShape(**dict(dict(up=4, site_len=23, down=3, gc_start=0, gc_len=0, link=0), **k))  # noqa: E731
    assert _build([STUMP], shape=ok(link=1)) == 0
    for bad in (ok(up=17), ok(down=17), ok(site_len=15), ok(site_len=33), ok(link=2), ok(gc_len=20), ok(gc_start=1)):
        assert _build([STUMP], shape=bad) == -22
    s = ok()
    s.reserved[1] = 1
    assert _build([STUMP], shape=s) == -22
    assert _build([[_node(1, a=63, mask=1, left=1, right=2), LEAF, LEAF]], shape=ok(up=16, site_len=32, down=16)) == 0  # C = 64
    for bad in (math.nan, math.inf, -math.inf):
        assert _build([STUMP], base=bad) == -22
    assert _build([[LEAF]] * 1025) == -22                                      # 1 025 trees
    assert _build([[LEAF]], n_trees=0) == -22                                  # no tree
    assert _build([STUMP, [LEAF]], first=[0, 3, 3], n_trees=2) == -22          # a tree without a node
    assert _build([STUMP, [LEAF]], first=[1, 3, 4], n_trees=2) == -22          # the first tree does not start at 0
    L, h = va.lib(), C.c_void_p()
    nodes, first = np.array([LEAF], dtype=_lib.EFF_NODE_DTYPE), np.array([0, 1], dtype=np.uint32)
    assert L.vsc_eff_trees_build(C.byref(ok()), 0.0, None, 0, _lib.ptr(nodes), _lib.ptr(first), 1, C.byref(h)) == 0
    L.vsc_eff_trees_free(h)
    assert L.vsc_eff_trees_build(C.byref(ok()), 0.0, None, 0, None, _lib.ptr(first), 1, C.byref(h)) == -22
    assert L.vsc_eff_trees_build(C.byref(ok()), 0.0, None, 0, _lib.ptr(nodes), None, 1, C.byref(h)) == -22
    assert L.vsc_eff_trees_build(None, 0.0, None, 0, _lib.ptr(nodes), _lib.ptr(first), 1, C.byref(h)) == -22
    assert L.vsc_eff_trees_build(C.byref(ok()), 0.0, None, 1, _lib.ptr(nodes), _lib.ptr(first), 1, C.byref(h)) == -22  # sums missing
    assert L.vsc_eff_trees_build(C.byref(ok()), 0.0, None, 0, _lib.ptr(nodes), _lib.ptr(first), 1, None) == -22


def test_the_wrapper_refuses_what_never_reaches_the_library():
    stump = lambda *test: [[test + (1, 2), ("leaf", 1.0), ("leaf", 2.0)]]  # noqa: E731
    va.TreeEfficiencyModel(4, 23, 3, 0.0, [], stump("base", 0, "ag"))
    for sums, trees in (([], stump("base", 0, "AN")), ([], stump("base", 0, "AA")), ([], stump("pair", 0, 1, ["A"])),
                        ([], stump("pair", 0, 1, "AC,ACG")), ([], [[("leaf",)]]), ([], [[("twig", 1.0)]]), ([], stump("base", 0.5, "A")),
                        ([(0, 30, {"ACG": 1})], stump("base", 0, "A")), ([(0, 30, {"N": 1})], stump("base", 0, "A")),
                        ([(0, 30, {"A": 2 ** 31})], stump("base", 0, "A")), ([(0, 30, {"A": 1})], stump("sum", 0, 2 ** 31))):
        with pytest.raises(ValueError):
            va.TreeEfficiencyModel(4, 23, 3, 0.0, sums, trees)
    with pytest.raises(ValueError):
        va.TreeEfficiencyModel(4, 23, 3, 0.0, [], stump("base", 0, "A"), link="probit")
    with pytest.raises(va.VarscotError):  # ... and what does: the library's refusal comes through
        va.TreeEfficiencyModel(4, 23, 3, 0.0, [], stump("base", 30, "A"))
    with pytest.raises(va.VarscotError):
        va.TreeEfficiencyModel(4, 23, 3, 0.0, [], [])
    m = tc.build("leaf1", (4, 23, 3))
    va.Genome._eff_args(m, -1.0, 23)
    with pytest.raises(ValueError):
        va.Genome._eff_args(m, None, 27)
    L, x = va.lib(), C.c_double()
    assert L.vsc_eff_trees_score_text(None, b"A" * 30, C.byref(x)) == -22 and L.vsc_eff_trees_score_text(m._h, None, C.byref(x)) == -22
    assert L.vsc_eff_trees_score_text(m._h, b"A" * 30, None) == -22
    assert L.vsc_eff_trees_info(m._h, None) == -22 and L.vsc_eff_trees_free(None) == 0
    assert tc.bits(L.vsc_eff_trees_link(None, 1.0)) == tc.UNDEF


# ---- zeros and the link --------------------------------------------------------------------------------------------------------
def test_negative_zero_is_stored_as_positive_zero():
    assert tc.bits(-0.0) == 1 << 63
    m = va.TreeEfficiencyModel(4, 23, 3, -0.0, [], [[("leaf", -0.0)], [("base", 0, "A", 1, 2), ("leaf", -0.0), ("leaf", -0.0)]])
    assert tc.bits(m.score_text("A" * 30)) == 0 and tc.bits(m.score_text("T" * 30)) == 0
    m2 = tc.build("leaf1", (4, 23, 3))
    assert m2.info()["serial"] > m.info()["serial"] > 0


def test_link_is_the_c_librarys_logistic():
    ident, logi = tc.build("azimuth", (4, 23, 3)), tc.build("azimuth", (4, 23, 3), link="logistic")
    assert logi.info()["link"] == "logistic"
    rng = np.random.default_rng(5)
    xs = [0.0, -0.0, 1.0, -1.0, 0.4921, 36.5, -36.5, 700.0, -700.0] + list(rng.normal(scale=3.0, size=200))
    for x in xs:
        assert tc.bits(ident.link(x)) == tc.bits(float(x))
        assert tc.bits(logi.link(x)) == tc.bits(1.0 / (1.0 + math.exp(-float(x)))), x
    assert logi.link(-800.0) == 0.0 and logi.link(800.0) == 1.0
    for m in (ident, logi):
        for nan in (math.nan, -math.nan, m.score_text("N" * 30)):
            assert tc.bits(m.link(nan)) == tc.UNDEF
    got = logi.link(np.array([[0.0, 1.0], [math.nan, -2.0]]))
    assert got.shape == (2, 2) and got[0, 0] == 0.5 and tc.bits(float(got[1, 0])) == tc.UNDEF
    t = _texts(30)[0]
    assert tc.bits(ident.score_text(t)) == tc.bits(logi.score_text(t))  # the link is the host's: the predictor is linear


# ---- the model file ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [f for f in tc.FAMILIES if f != "largest"])
def test_tsv_round_trip(tmp_path, family):
    shape = (6, 23, 6)
    model = tc.lists(family, shape)
    m = tc.build(family, shape, link="logistic")
    path = tmp_path / "model.tsv"
    m.to_tsv(path)
    assert any(line.split()[:1] == ["tree"] for line in path.read_text().splitlines())
    back = va.TreeEfficiencyModel.from_tsv(path)
    assert (back.up, back.site_len, back.down, back.link_name) == (6, 23, 6, "logistic")
    assert tc.bits(back.base) == tc.bits(m.base) and back.sums == m.sums
    a, b = back.info(), m.info()
    assert {k: v for k, v in a.items() if k != "serial"} == {k: v for k, v in b.items() if k != "serial"}
    assert [tc.bits(n[1]) for t in back.trees for n in t if n[0] == "leaf"] == [tc.bits(n[1]) for t in m.trees for n in t if n[0] == "leaf"]
    for t in _texts(sum(shape), n=10, seed=9):
        assert tc.bits(back.score_text(t)) == tc.bits(m.score_text(t)) == tc.py_predict_bits(model, t)
    again = tmp_path / "again.tsv"
    back.to_tsv(again)
    assert again.read_bytes() == path.read_bytes()


GOOD_TSV = ["# a comment", "shape 4 23 3", "link identity", "intercept 0.25", "sum 0 4 20", "sumw 0 G 1", "sumw 0 GC -2", "tree 0",
            "base_in 0 0 AG 1 2", "leaf 1 1.5", "sum_le 2 0 10 3 4", "leaf 3 -2", "pair_in 4 5 3 AC,GT 5 6", "leaf 5 0.125", "leaf 6 1e-3",
            "tree 1", "leaf 0 7", ""]


def test_tsv_parse_and_refusals(tmp_path):
    path = tmp_path / "m.tsv"

    def load(lines):
        path.write_text("\n".join(lines) + "\n")
        return va.TreeEfficiencyModel.from_tsv(path)

    m = load(GOOD_TSV)
    assert m.base == 0.25 and m.sums == [(4, 20, {"G": 1, "GC": -2})] and len(m.trees) == 2 and m.trees[1] == [("leaf", 7.0)]
    assert m.trees[0][4] == ("pair", 5, 3, "AC,GT", 5, 6) and m.info()["n_nodes"] == 8
    assert m.score_text("A" * 30) == 0.25 + 1.5 + 7.0
    bad = [(7, "sumw 0 G 3"),            # a weight given twice
           (5, "sumw 1 A 3"),            # a weight before its sum
           (5, "sumw 0 ACG 3"),
           (5, "sumw 0 N 3"),
           (5, "sumw 0 A 1.5"),          # no integer
           (5, "sum 2 0 4"),             # a sum out of turn
           (5, "sum 0 0 4"),
           (5, "leaf 0 1.0"),            # a node before the first tree
           (5, "mono 0 A 1.5"),          # a linear model's line
           (5, "gc_range 4 20"),
           (5, "colour 0 A 1.5"),        # an unknown key
           (9, "leaf 2 1.0"),            # a node out of turn
           (9, "leaf 0 1.0"),
           (9, "leaf 1"),                # a field too few
           (9, "leaf 1 one"),
           (9, "base_in 1 0 AN 2 3"),    # no base
           (9, "base_in 1 0 AA 2 3"),    # a letter given twice
           (9, "pair_in 1 0 1 ACG 2 3"),
           (9, "pair_in 1 0 1 AC 2"),
           (9, "sum_le 1 0 1.5 2 3"),
           (9, "tree 2"),                # a tree out of turn
           (8, "tree 1"),                # a tree without a node
           (3, "shape 4 23 3"),          # a key given twice
           (2, "link probit"),
           (1, "shape 4 23")]
    for at, line in bad:
        lines = GOOD_TSV[:at] + [line] + GOOD_TSV[at:]
        with pytest.raises(ValueError) as e:
            load(lines)
        assert str(e.value).startswith("%s:%d:" % (path, at + 1)), (line, str(e.value))
    with pytest.raises(ValueError) as e:
        load(["intercept 1.0", "tree 0", "leaf 0 1"])
    assert "no 'shape' line" in str(e.value)
    with pytest.raises(ValueError) as e:
        load(["shape 4 23 3"])
    assert "no 'tree' line" in str(e.value)
    with pytest.raises(va.VarscotError):  # a structure the library refuses
        load(["shape 4 23 3", "tree 0", "base_in 0 30 A 1 2", "leaf 1 1", "leaf 2 1"])
    assert load(["shape 4 23 3", "tree 0", "base_in 0 0 - 1 2", "leaf 1 1", "leaf 2 2"]).score_text("A" * 30) == 2.0  # '-': no letter


# ---- two cross-checks against the linear model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("with_di", [False, True], ids=["mono", "mono+di"])
def test_stumps_equal_the_linear_model(with_di):
    """C * 4 BASE stumps in (position, letter) order with leaves (w, +0.0) - and behind them (C - 1) * 16 PAIR stumps on
    adjacent positions - add up the linear model's terms in its order; adding +0.0 is exact (no sum is -0.0: -0.0 is stored
    as +0.0 on both sides)."""
    shape = (4, 23, 3)
    C_ = 30
    a = ec.arrays("mixed", shape)
    di = a["di"] if with_di else np.zeros((C_ - 1, 16))
    linear = va.EfficiencyModel(4, 23, 3, a["intercept"], a["mono"], di)
    trees = [[("base", j, "ACGT"[b], 1, 2), ("leaf", float(a["mono"][j, b])), ("leaf", 0.0)] for j in range(C_) for b in range(4)]
    if with_di:
        trees += [[("pair", j, j + 1, [tc.DINUCS[d]], 1, 2), ("leaf", float(di[j, d])), ("leaf", 0.0)] for j in range(C_ - 1) for d in range(16)]
    m = va.TreeEfficiencyModel(4, 23, 3, a["intercept"], [], trees)
    for t in _texts(C_, n=60):
        assert tc.bits(m.score_text(t)) == ec.bits(linear.score_text(t)), t


# ---- scikit-learn --------------------------------------------------------------------------------------------------------------
def _sklearn_problem(n=4000, C_=30, seed=3):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, size=(n, C_))
    texts = ["".join("ACGT"[b] for b in row) for row in codes]
    features = [("base", j, "ACGT"[b]) for j in range(C_) for b in range(4)] + [("sum", i) for i in range(5)]
    sums = [(4, 20, {"G": 1, "C": 1})] + [(0, C_, {ch: 1}) for ch in "ACGT"]
    X = np.zeros((n, len(features)))
    for j in range(C_):
        for b in range(4):
            X[:, 4 * j + b] = codes[:, j] == b
    X[:, 120] = np.isin(codes[:, 4:24], (1, 2)).sum(axis=1)
    for b in range(4):
        X[:, 121 + b] = (codes == b).sum(axis=1)
    w = rng.normal(size=len(features)) * ([1.0] * 120 + [0.3] * 5)
    y = X @ w + 0.5 * X[:, 7] * X[:, 90] + rng.normal(scale=0.1, size=n)
    return texts, features, sums, X, y


def test_sklearn_conversion_is_bit_exact():
    ensemble = pytest.importorskip("sklearn.ensemble")
    texts, features, sums, X, y = _sklearn_problem()
    est = ensemble.GradientBoostingRegressor(n_estimators=100, max_depth=3, random_state=0).fit(X, y)
    m = va.TreeEfficiencyModel.from_sklearn(est, features, 4, 23, 3, sums=sums)
    info = m.info()
    assert info["n_trees"] == 100 and info["max_depth"] == 3 and info["sum_nodes"] > 0 and info["base_nodes"] > 0
    want = est.predict(X)
    got = np.array([m.score_text(t) for t in texts])
    assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist()
    zero = ensemble.GradientBoostingRegressor(n_estimators=5, max_depth=2, init="zero", random_state=0).fit(X[:500], y[:500])
    mz = va.TreeEfficiencyModel.from_sklearn(zero, features, 4, 23, 3, sums=sums)
    assert mz.base == 0.0
    assert np.array([mz.score_text(t) for t in texts[:500]]).view(np.uint64).tolist() == zero.predict(X[:500]).view(np.uint64).tolist()


def test_sklearn_refusals():
    ensemble = pytest.importorskip("sklearn.ensemble")
    texts, features, sums, X, y = _sklearn_problem(n=300)
    with pytest.raises(ValueError):
        va.TreeEfficiencyModel.from_sklearn(ensemble.RandomForestRegressor(n_estimators=3, random_state=0).fit(X, y), features, 4, 23, 3, sums=sums)
    huber = ensemble.GradientBoostingRegressor(n_estimators=3, loss="huber", random_state=0).fit(X, y)
    with pytest.raises(ValueError):
        va.TreeEfficiencyModel.from_sklearn(huber, features, 4, 23, 3, sums=sums)
    with pytest.raises(ValueError):  # not fitted
        va.TreeEfficiencyModel.from_sklearn(ensemble.GradientBoostingRegressor(), features, 4, 23, 3, sums=sums)
    est = ensemble.GradientBoostingRegressor(n_estimators=3, random_state=0).fit(X, y)
    with pytest.raises(ValueError):  # a column without a name
        va.TreeEfficiencyModel.from_sklearn(est, features[:-1], 4, 23, 3, sums=sums)
    with pytest.raises(ValueError):
        va.TreeEfficiencyModel.from_sklearn(est, [("gc", 1)] * len(features), 4, 23, 3, sums=sums)
    with pytest.raises(ValueError):  # its own regressor as init
        other = ensemble.GradientBoostingRegressor(n_estimators=3, init=ensemble.RandomForestRegressor(n_estimators=2, random_state=0), random_state=0)
        va.TreeEfficiencyModel.from_sklearn(other.fit(X, y), features, 4, 23, 3, sums=sums)


def test_sklearn_splits_on_indicators_and_sums():
    """The conversion rules one by one, on a hand-made stand-in for the fitted trees (no training involved)."""
    pytest.importorskip("sklearn.ensemble")
    from sklearn.ensemble import GradientBoostingRegressor

    rng = np.random.default_rng(1)
    X = rng.integers(0, 2, size=(200, 3)).astype(float)
    X[:, 2] = rng.integers(0, 9, size=200)
    est = GradientBoostingRegressor(n_estimators=4, max_depth=2, random_state=0).fit(X, X[:, 0] + 2 * X[:, 1] * (X[:, 2] > 3.5) + 0.1 * X[:, 2])
    features = [("base", 2, "G"), ("pair", 9, 4, "TA"), ("sum", 0)]
    m = va.TreeEfficiencyModel.from_sklearn(est, features, 4, 23, 3, sums=[(10, 8, {"C": 1})])
    kinds = {n[0] for t in m.trees for n in t}
    assert kinds == {"leaf", "base", "pair", "sum"}
    for t in m.trees:
        for n in t:
            if n[0] == "base":
                assert n[1:3] == (2, "ACT")                       # x <= 0.5 is "the letter is not G"
            elif n[0] == "pair":
                assert n[1:3] == (9, 4) and len(n[3]) == 15 and "TA" not in n[3]
            elif n[0] == "sum":
                assert n[2] == math.floor(n[2]) and 0 <= n[2] < 8
    for _ in range(200):
        text = random_seq(rng, 30)
        row = np.array([[text[2] == "G", text[9] + text[4] == "TA", text[10:18].count("C")]], dtype=float)
        assert tc.bits(m.score_text(text)) == tc.bits(float(est.predict(row)[0]))

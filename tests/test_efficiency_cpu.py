"""The host side of the on-target efficiency score (include/varscot_hip.h "on-target efficiency"), without a device:
vsc_eff_score_text - the function the kernels run - against the Python restatement to the bit, every refusal of
vsc_eff_model_build, the -0.0 normalisation, the link, the TSV form and from_features."""
import ctypes as C
import math

import numpy as np
import pytest

import efficiency_cases as ec
import varscot_amd as va
from helpers import random_seq
from varscot_amd import _lib


@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "%d-%d-%d" % s)
@pytest.mark.parametrize("family", ec.FAMILIES)
def test_score_text_equals_the_restatement(family, shape):
    a = ec.arrays(family, shape)
    m = ec.build(family, shape)
    C_ = sum(shape)
    rng = np.random.default_rng(7)
    texts = [random_seq(rng, C_) for _ in range(40)] + ["A" * C_, "C" * C_, "G" * C_, "T" * C_, ("ACGT" * 16)[:C_]]
    texts.append(texts[0].lower())
    for t in texts:
        assert ec.bits(m.score_text(t)) == ec.py_linear_bits(a, t), t
    for at in (0, C_ // 2, C_ - 1):  # a letter outside ACGT, anywhere: undefined, the one NaN
        t = texts[1][:at] + "N" + texts[1][at + 1:]
        assert ec.bits(m.score_text(t)) == ec.UNDEF
    for t in (texts[0][:-1], texts[0] + "A", ""):  # another length is refused
        with pytest.raises(va.VarscotError) as e:
            m.score_text(t)
        assert e.value.code == -22
    info = m.info()
    assert (info["up"], info["site_len"], info["down"]) == shape and info["link"] == "identity"
    assert info["nonzero_weights"] == sum(int(np.count_nonzero(a[k])) for k in ("mono", "di", "gc") if a[k] is not None)


def test_the_order_of_the_additions_shows_in_the_mixed_family():
    """The family exists so that a reassociated sum is caught: summing mono and di interleaved gives other bits somewhere."""
    shape = (4, 23, 3)
    a = ec.arrays("mixed", shape)
    rng = np.random.default_rng(3)
    differs = 0
    for _ in range(40):
        t = random_seq(rng, sum(shape))
        b = ["ACGT".index(ch) for ch in t]
        x = float(a["intercept"])
        for j in range(len(b)):
            x = x + float(a["mono"][j][b[j]])
            if j + 1 < len(b):
                x = x + float(a["di"][j][4 * b[j] + b[j + 1]])
        s, n = a["gc_range"]
        x = x + float(a["gc"][sum(ch in "GC" for ch in t[s:s + n])])
        differs += ec.bits(x) != ec.py_linear_bits(a, t)
    assert differs > 0


def _build(shape, intercept, mono, di, gc):
    h = C.c_void_p()
    code = va.lib().vsc_eff_model_build(C.byref(shape), float(intercept), _lib.ptr(mono), _lib.ptr(di), _lib.ptr(gc), C.byref(h))
    if code == 0:
        va.lib().vsc_eff_model_free(h)
    else:
        assert not h.value
    return code


def test_model_build_refusals():
    C_ = 30
    mono, di, gc = np.zeros((C_, 4)), np.zeros((C_ - 1, 16)), np.zeros(21)
    ok = lambda **k: _lib.EffShape(**dict(dict(up=4, site_len=23, down=3, gc_start=4, gc_len=20, link=0), **k))  # noqa: E731
    assert _build(ok(), 0.0, mono, di, gc) == 0
    for bad in (np.nan, np.inf, -np.inf):  # a weight that is not finite, in every array and the intercept
        for which in range(4):
            arrs = [mono.copy(), di.copy(), gc.copy()]
            icpt = 0.0
            if which < 3:
                arrs[which].reshape(-1)[-1] = bad
            else:
                icpt = bad
            assert _build(ok(), icpt, *arrs) == -22
    big_m, big_d = np.zeros((80, 4)), np.zeros((79, 16))
    assert _build(ok(up=16, site_len=32, down=16), 0.0, big_m, big_d, gc) == 0                      # C = 64
    assert _build(ok(up=16, site_len=32, down=16, gc_start=44, gc_len=20), 0.0, big_m, big_d, gc) == 0  # the range ends with the context
    assert _build(ok(up=16, site_len=32, down=16, gc_start=45, gc_len=20), 0.0, big_m, big_d, gc) == -22
    assert _build(ok(up=17, site_len=23, down=0), 0.0, big_m, big_d, gc) == -22                     # a flank > 16
    assert _build(ok(up=0, site_len=23, down=17), 0.0, big_m, big_d, gc) == -22
    assert _build(ok(up=4, site_len=15, down=3), 0.0, big_m, big_d, gc) == -22                      # site_len outside 16..32
    assert _build(ok(up=4, site_len=33, down=3), 0.0, big_m, big_d, gc) == -22
    assert _build(ok(up=16, site_len=32, down=16, gc_start=0xFFFFFFF0, gc_len=20), 0.0, big_m, big_d, gc) == -22  # no wrap-around
    assert _build(ok(gc_start=11, gc_len=20), 0.0, mono, di, gc) == -22                             # the G/C range leaves the context
    assert _build(ok(gc_start=31, gc_len=0), 0.0, mono, di, None) == -22
    assert _build(ok(gc_len=0), 0.0, mono, di, gc) == -22                                           # gc given with gc_len == 0
    assert _build(ok(), 0.0, mono, di, None) == -22                                                 # ... and the reverse
    assert _build(ok(gc_len=0), 0.0, mono, di, None) == 0
    assert _build(ok(link=2), 0.0, mono, di, gc) == -22
    for k in (0, 1):                                                                                # a reserved field that is not 0
        s = ok()
        s.reserved[k] = 1
        assert _build(s, 0.0, mono, di, gc) == -22
    assert _build(ok(), 0.0, None, di, gc) == -22 and _build(ok(), 0.0, mono, None, gc) == -22
    assert va.lib().vsc_eff_model_build(C.byref(ok()), 0.0, _lib.ptr(mono), _lib.ptr(di), _lib.ptr(gc), None) == -22
    with pytest.raises(ValueError):  # the wrapper: arrays of another shape never reach the library
        va.EfficiencyModel(4, 23, 3, 0.0, np.zeros((29, 4)), di)
    with pytest.raises(ValueError):
        va.EfficiencyModel(4, 23, 3, 0.0, mono, di, gc=gc)
    with pytest.raises(ValueError):
        va.EfficiencyModel(4, 23, 3, 0.0, mono, di, link="probit")


def test_negative_zero_is_stored_as_positive_zero():
    """-0.0 + -0.0 is -0.0: only the normalisation makes the sum of an all -0.0 model +0.0 - and then x is never -0.0, so
    that an implementation may skip the terms that are exactly 0."""
    C_ = 30
    nz = lambda *shape: np.full(shape, -0.0)  # noqa: E731
    assert ec.bits(float(nz(1)[0])) == 1 << 63
    m = va.EfficiencyModel(4, 23, 3, -0.0, nz(C_, 4), nz(C_ - 1, 16), gc=nz(21), gc_range=(4, 20))
    assert ec.bits(m.score_text("ACGT" * 7 + "AC")) == 0
    assert m.info()["nonzero_weights"] == 0
    m2 = va.EfficiencyModel(4, 23, 3, -0.0, nz(C_, 4), nz(C_ - 1, 16))
    assert ec.bits(m2.score_text("T" * C_)) == 0
    assert m2.info()["serial"] > m.info()["serial"] > 0


def test_link_is_the_c_librarys_logistic():
    ident, logi = ec.build("dense", (4, 23, 3)), ec.build("dense", (4, 23, 3), link="logistic")
    assert logi.info()["link"] == "logistic"
    rng = np.random.default_rng(5)
    xs = [0.0, -0.0, 1.0, -1.0, 0.59763615, 36.5, -36.5, 700.0, -700.0] + list(rng.normal(scale=3.0, size=200))
    for x in xs:
        assert ec.bits(ident.link(x)) == ec.bits(float(x))
        assert ec.bits(logi.link(x)) == ec.bits(ec.py_logistic(float(x))), x
    assert logi.link(-800.0) == 0.0 and logi.link(800.0) == 1.0  # exp overflows to inf: 1 / inf
    for m in (ident, logi):  # link(undefined) = undefined, whatever NaN comes in
        for nan in (math.nan, -math.nan, m.score_text("N" * 30)):
            assert ec.bits(m.link(nan)) == ec.UNDEF
    got = logi.link(np.array([[0.0, 1.0], [math.nan, -2.0]]))
    assert got.shape == (2, 2) and got[0, 0] == 0.5 and ec.bits(float(got[1, 0])) == ec.UNDEF


@pytest.mark.parametrize("family", ec.FAMILIES)
def test_tsv_round_trip(tmp_path, family):
    shape = (6, 23, 6)
    a = ec.arrays(family, shape)
    m = ec.build(family, shape, link="logistic")
    path = tmp_path / "model.tsv"
    m.to_tsv(path)
    back = va.EfficiencyModel.from_tsv(path)
    assert (back.up, back.site_len, back.down, back.link_name, back.gc_range) == (6, 23, 6, "logistic", a["gc_range"])
    assert back.intercept == m.intercept and back.mono.tobytes() == m.mono.tobytes() and back.di.tobytes() == m.di.tobytes()
    assert (back.gc is None) == (m.gc is None) and (m.gc is None or back.gc.tobytes() == m.gc.tobytes())
    rng = np.random.default_rng(9)
    for _ in range(10):
        t = random_seq(rng, sum(shape))
        assert ec.bits(back.score_text(t)) == ec.bits(m.score_text(t)) == ec.py_linear_bits(a, t)


GOOD_TSV = ["# a comment", "shape 4 23 3", "link identity", "intercept 0.25", "gc_range 4 20", "mono 0 A 1.5", "di 28 GT -2", "gc 20 0.125", ""]


def test_tsv_parse_and_refusals(tmp_path):
    path = tmp_path / "m.tsv"

    def load(lines):
        path.write_text("\n".join(lines) + "\n")
        return va.EfficiencyModel.from_tsv(path)

    m = load(GOOD_TSV)
    assert m.intercept == 0.25 and m.mono[0, 0] == 1.5 and m.di[28, 4 * 2 + 3] == -2.0 and m.gc[20] == 0.125
    assert np.count_nonzero(m.mono) + np.count_nonzero(m.di) + np.count_nonzero(m.gc) == 3 == m.info()["nonzero_weights"]
    bad = [(6, "mono 0 A 1.5"),        # a feature given twice
           (6, "mono 0 a 2.5"),
           (5, "colour 0 A 1.5"),      # an unknown key
           (5, "mono 0 A"),            # a field too few
           (5, "mono 0 AC 1.0"),       # mono takes one letter
           (5, "di 0 A 1.0"),
           (5, "di 29 AC 1.0"),        # the dinucleotide leaves the context
           (5, "mono 30 A 1.0"),
           (5, "mono -1 A 1.0"),
           (5, "mono 0 N 1.0"),        # no base
           (5, "mono 0 A one"),        # no number
           (5, "gc 21 1.0"),           # a count the range cannot reach
           (8, "gc 20 3.0"),           # a count given twice
           (3, "shape 4 23 3"),        # a key given twice
           (2, "link probit"),
           (1, "shape 4 23")]
    for at, line in bad:
        lines = GOOD_TSV[:at] + [line] + GOOD_TSV[at:]
        with pytest.raises(ValueError) as e:
            load(lines)
        assert str(e.value).startswith("%s:%d:" % (path, at + 1)), (line, str(e.value))
    with pytest.raises(ValueError) as e:  # a weight before its shape
        load(["# c", "mono 0 A 1.5", "shape 4 23 3"])
    assert str(e.value).startswith("%s:2:" % path)
    with pytest.raises(ValueError) as e:  # gc before gc_range
        load(["shape 4 23 3", "gc 1 1.0"])
    assert str(e.value).startswith("%s:2:" % path)
    with pytest.raises(ValueError) as e:  # no shape at all
        load(["intercept 1.0"])
    assert "no 'shape' line" in str(e.value)
    with pytest.raises(va.VarscotError):  # a shape the library refuses
        load(["shape 17 23 3"])


def test_from_features_against_dense_arrays():
    shape = (4, 23, 3)
    a = ec.arrays("sparse", shape)
    feats = [(int(j), "ACGT"[b], float(a["mono"][j, b])) for j, b in zip(*np.nonzero(a["mono"]))]
    feats += [(int(j), "ACGT"[d // 4] + "ACGT"[d % 4], float(a["di"][j, d])) for j, d in zip(*np.nonzero(a["di"]))]
    assert 60 <= len(feats) <= 80
    feats = [feats[k] for k in np.random.default_rng(1).permutation(len(feats))]  # the order of the list does not matter
    m = va.EfficiencyModel.from_features(4, 23, 3, a["intercept"], feats, gc=a["gc"], gc_range=a["gc_range"])
    assert m.mono.tobytes() == a["mono"].tobytes() and m.di.tobytes() == a["di"].tobytes()
    dense = ec.build("sparse", shape)
    rng = np.random.default_rng(2)
    for _ in range(20):
        t = random_seq(rng, 30)
        assert ec.bits(m.score_text(t)) == ec.bits(dense.score_text(t)) == ec.py_linear_bits(a, t)
    lower = va.EfficiencyModel.from_features(4, 23, 3, 0.0, [(3, "g", 1.0), (3, "gu", 2.0)])  # any case, U for T
    assert lower.mono[3, 2] == 1.0 and lower.di[3, 4 * 2 + 3] == 2.0
    for bad in ([(0, "A", 1.0), (0, "a", 2.0)], [(0, "AC", 1.0), (0, "AC", 1.0)], [(30, "A", 1.0)], [(29, "AC", 1.0)], [(-1, "A", 1.0)],
                [(0, "ACG", 1.0)], [(0, "", 1.0)], [(0, "N", 1.0)]):
        with pytest.raises(ValueError):
            va.EfficiencyModel.from_features(4, 23, 3, 0.0, bad)


def test_arguments_the_wrappers_refuse():
    m = ec.build("zero", (4, 23, 3))
    with pytest.raises(ValueError):
        va.Genome._eff_args(None, 1.0, 23)              # a floor without a model
    with pytest.raises(ValueError):
        va.Genome._eff_args(m, None, 27)                # a model for sites of another length
    with pytest.raises(ValueError):
        va.Genome._eff_args("model.tsv", None, 23)
    va.Genome._eff_args(m, -1.0, 23)
    L = va.lib()
    x = C.c_double()
    assert L.vsc_eff_score_text(None, b"A" * 30, C.byref(x)) == -22 and L.vsc_eff_score_text(m._h, None, C.byref(x)) == -22
    assert L.vsc_eff_score_text(m._h, b"A" * 30, None) == -22
    assert L.vsc_eff_model_info(m._h, None) == -22 and L.vsc_eff_model_free(None) == 0
    assert ec.bits(L.vsc_eff_link(None, 1.0)) == ec.UNDEF

"""The host side of the variation join (vsc_variation_host, the shape and its presets, site_variants' normalisation, the weight
helper, variation_pick_inputs, every validation error, the stand-alone check program): the library against the strings and lists
of tests/variation_cases.py, as integers.  No device is needed."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import edit_cases as ed
import variation_cases as vc
import varscot_amd as va
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ["none", "one", "one_contig", "third", "every3", "edges", "ends", "saturated"]


@pytest.mark.parametrize("which", SETS)
@pytest.mark.parametrize("shape_name", sorted(vc.SHAPES))
def test_the_host_definition_at_every_locus_of_the_small_genome(shape_name, which):
    shape = vc.SHAPES[shape_name]()
    contigs = ed.small_genome(shape[0])
    variants, _ = vc.variant_sets(contigs, shape[0])[which]
    loci = ed.every_locus(contigs) + ed.invalid_loci(contigs)  # every (contig, p, strand), both strands
    want = vc.expected(contigs, loci, shape, variants, planes=False)
    rows, pairs, cov = va.variation_host(vc.contig_array(contigs), ed.locus_array(loci), vc.shape_of(shape), vc.variant_array(variants), coverage=True)
    assert rows.dtype == np.uint32 and rows.shape == (len(loci), 4) and rows.tobytes() == want["rows"].tobytes()
    assert pairs.dtype == va.VARIATION_PAIR_DTYPE and pairs.tobytes() == want["pairs"].tobytes()
    assert cov.tobytes() == want["coverage"].tobytes()
    assert want["stats"]["has_n"] == 0 and want["stats"]["invalid"] > 20 and want["stats"]["defined"] > 1000  # no planes: two classes
    if which != "none":
        assert len(pairs) > 0
    # rows given in the caller's form and in any order come back in the caller's numbering
    if which == "third":
        perm = [int(i) for i in np.random.default_rng(4).permutation(len(variants))]
        given = [(variants[i][0], variants[i][1], contigs[variants[i][0]][variants[i][1]], variants[i][3], variants[i][4]) for i in perm]
        r2, p2, c2 = va.variation_host(vc.contig_array(contigs), ed.locus_array(loci), vc.shape_of(shape), given, coverage=True)
        back = want["pairs"].copy()
        back["variant"] = np.argsort(perm).astype(np.uint32)[back["variant"].astype(np.int64)]  # sorted variant k was given as row argsort(perm)[k]
        back = back[np.lexsort((back["variant"], back["candidate"]))]
        assert r2.tobytes() == rows.tobytes() and p2.tobytes() == back.tobytes() and c2.tobytes() == cov[perm].tobytes()


def test_the_cases_hold_what_they_are_for():
    contigs = ed.small_genome()
    assert [len(c) for c in contigs] == [22, 23, 24, 700, 500]
    sets = vc.variant_sets(contigs, 23)
    for name, (variants, _) in sets.items():
        assert variants == vc.ordered(variants), name  # ascending (contig, pos), ties in their order
        for c, p, span, alt, w in variants:
            assert 0 <= p and p + span <= len(contigs[c]) and (alt is None or span == 1) and 0 <= w <= vc.MAX_U32
    every = sets["every3"][0]
    assert sum(1 for v in every if (v[0], v[1]) == (ed.MAIN, 200)) == 3 and len({v[3] for v in every if (v[0], v[1]) == (ed.MAIN, 200)}) == 3
    assert all(v[3] != contigs[v[0]][v[1]] for v in every)  # an alt is not the reference's letter
    spans = {(v[1], v[2]) for v in sets["edges"][0]}
    assert all((200 - s, s) in spans and (223, s) in spans and (201 - s, s) in spans and (222, s) in spans for s in range(1, 41))
    assert sum(1 for v in sets["saturated"][0] if v[1] == 420) == 300


def test_site_variants_normalises_vcf_style_alleles():
    rows = [(0, 10, "A", "G"),            # an SNV
            (0, 20, "CAT", "C", 7),       # a deletion behind its anchor: the bases 21 and 22
            (0, 30, "C", "CGG"),          # an insertion behind its anchor: the bases 30 and 31 flank it
            (0, 40, "ACG", "TCA"),        # an MNV: A..G -> T..A, its length
            (0, 50, "GATTACA", "GATCACA"),  # an SNV inside equal flanks: prefix GAT and suffix ACA go
            (0, 60, "AC", "GCT"),         # anything else: the bases of what is left of ref
            (0, 0, "A", "TA"),            # an insertion in front of a contig's first base: that base alone
            (0, 70, "acgt", "a", 3),      # lower case
            (1, 5, "T", "N"),             # a substitution to no letter: alt 4
            (0, 10, "A", "T", 9), (0, 10, "A", "C", 8)]  # a multi-allelic site: ties keep their order
    var, order, inverse = va.site_variants(rows)
    assert var.dtype == va.VARIANT_DTYPE
    got = [(int(v["contig"]), int(v["pos"]), int(v["span_alt"]) & 0xFFFF, int(v["span_alt"]) >> 16, int(v["weight"])) for v in var]
    assert got == [(0, 0, 1, 4, 0), (0, 10, 1, 2, 0), (0, 10, 1, 3, 9), (0, 10, 1, 1, 8), (0, 21, 2, 4, 7), (0, 30, 2, 4, 0), (0, 40, 3, 4, 0),
                   (0, 53, 1, 1, 0), (0, 60, 2, 4, 0), (0, 71, 3, 4, 3), (1, 5, 1, 4, 0)]
    assert order.tolist() == [6, 0, 9, 10, 1, 2, 3, 4, 5, 7, 8] and [order[k] for k in inverse] == list(range(len(rows)))
    # rows given unsorted: the same array, the permutation says where each came from
    rng = np.random.default_rng(3)
    perm = [int(i) for i in rng.permutation(len(rows))]
    shuffled = [rows[i] for i in perm]
    var2, order2, _ = va.site_variants(shuffled)
    assert sorted(v.tobytes() for v in var2) == sorted(v.tobytes() for v in var) and [(v["contig"], v["pos"]) for v in var2] == [(v["contig"], v["pos"]) for v in var]
    for k, i in enumerate(order2):
        assert va.site_variants([shuffled[int(i)]])[0][0].tobytes() == var2[k].tobytes()
    # an insertion at a contig's end needs the lengths; without them it spans one base too many, which the library refuses
    assert [int(v["span_alt"]) & 0xFFFF for v in va.site_variants([(0, 99, "A", "AT")], lengths=[100])[0]] == [1]
    assert [int(v["span_alt"]) & 0xFFFF for v in va.site_variants([(0, 99, "A", "AT")])[0]] == [2]
    empty = va.site_variants([])
    assert len(empty[0]) == 0 and len(empty[1]) == 0 and len(empty[2]) == 0
    for bad in ([(0, 5, "A", "A")], [(0, 5, "AC", "AC")], [(0, 5, "A", "<DEL>")], [(0, 5, "A", "*")], [(0, 5, "", "A")], [(0, 5, "A", "")],
                [(-1, 5, "A", "C")], [(0, 2 ** 32, "A", "C")], [(0, 5, "A", "C", 0xFFFFFFFF)], [(0, 5, "A" * 65537, "A")], [(0, 5, "A")]):
        with pytest.raises(ValueError):
            va.site_variants(bad)
    assert (int(va.site_variants([(0, 5, "A" * 65536, "A")])[0][0]["span_alt"]) & 0xFFFF) == 65535


def test_the_weight_helper():
    for af, want in vc.weight_cases():
        assert va.variant_weight(af) == want, af
    afs = np.array([af for af, _ in vc.weight_cases()])
    assert va.variant_weight(afs).tolist() == [w for _, w in vc.weight_cases()] and va.variant_weight(afs).dtype == np.uint32
    assert va.variant_weight(0) == 0 and va.variant_weight(1.0) == 0xFFFFFFFE and va.variant_weight(1.5) == 0xFFFFFFFE
    assert va.variant_weight(1 - 1e-300) == 0xFFFFFFFE  # the scaled value is past the clamp
    assert va.VARIANT_WEIGHT_ONE == 2 ** 20 and va.variant_weight(1 - math.exp(-1)) == 2 ** 20
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError):
            va.variant_weight(bad)
    # under independence the cost is -ln P(no disrupting variant): two variants of 1 % and 5 %
    cost = va.variant_weight(0.01) + va.variant_weight(0.05)
    assert abs(va.carrier_free(cost) - 0.99 * 0.95) < 1e-6 and va.carrier_free(0) == 1.0
    assert va.carrier_free(np.array([0, 2 ** 20])).tolist() == [1.0, math.exp(-1)] and va.carrier_free(0xFFFFFFFE) < 1e-300


def test_shapes_presets_and_their_packing():
    sp = va.VARIATION_SHAPES["SpCas9"]
    assert [sp.zone(j) for j in range(23)] == [1] * 10 + [2] * 10 + [0, 3, 3] and [sp.accepts(j) for j in range(23)] == [0] * 20 + [15, 4, 4]
    st = sp._struct()
    assert C.sizeof(st) == 48 and st.site_len == 23 and st.reserved0 == 0 and list(st.reserved) == [0, 0, 0, 0]
    assert st.zones == sum(z << (2 * j) for j, z in enumerate([1] * 10 + [2] * 10 + [0, 3, 3]))
    assert st.accept[0] == 0 and st.accept[1] == 15 << 16 | 4 << 20 | 4 << 24  # positions 20, 21, 22 are nibbles 4, 5, 6 of the second word
    for name, case in (("SpCas9", vc.spcas9()), ("Cas12a", vc.cas12a27())):
        a, b = va.VARIATION_SHAPES[name]._struct(), vc.shape_of(case)._struct()
        assert (a.site_len, a.zones, list(a.accept)) == (b.site_len, b.zones, list(b.accept))
    sa = va.variation_shape_from_pattern("N" * 21 + "NNGRRT", (0, 21), 10)  # the R accepts A and G
    assert [sa.zone(j) for j in range(27)] == [1] * 11 + [2] * 10 + [0, 0, 3, 3, 3, 3] and [sa.accepts(j) for j in range(21, 27)] == [15, 15, 4, 5, 5, 8]
    assert va.variation_shape_from_pattern(b"TTTV" + b"N" * 23, (4, 23), 8).zones == va.VARIATION_SHAPES["Cas12a"].zones
    assert va.variation_shape_from_pattern("N" * 20 + "NGG", (0, 20), 0).zones == sum(1 << (2 * j) for j in range(20)) | 15 << 42
    assert repr(sp).startswith("VariationShape(site_len=23, zones='11111111112222222222033'")
    for kw in (dict(site_len=15), dict(site_len=33), dict(zones=1 << 46), dict(accept=(0, 1 << 28)), dict(site_len=16, accept=(0, 1)),
               dict(zones=[1] * 22), dict(zones=[4] + [0] * 22), dict(accept=["A"] * 22), dict(accept=[16] + [0] * 22), dict(zones=-1)):
        with pytest.raises(ValueError):
            va.VariationShape(**kw)
    with pytest.raises(KeyError):
        va.VariationShape(accept=["Z"] + [""] * 22)
    for bad in (("N" * 23, (0, 24), 5), ("N" * 23, (0, 20), 21), ("NG" + "N" * 19 + "GG", (2, 19), 5), ("N" * 20 + "NG!", (0, 20), 5)):
        with pytest.raises(ValueError):
            va.variation_shape_from_pattern(*bad)
    assert va.VariationShape(32, [3] * 32, ["N"] * 32)._struct().zones == 2 ** 64 - 1


def test_struct_sizes_and_unpacking():
    assert C.sizeof(_lib.VariationShapeStruct) == 48 and C.sizeof(_lib.VariationFilterStruct) == 16 and C.sizeof(_lib.VariationStats) == 96
    assert va.VARIANT_DTYPE.itemsize == 16 and va.VARIANT_DTYPE.names == ("contig", "pos", "span_alt", "weight")
    assert va.VARIATION_PAIR_DTYPE.itemsize == 16 and va.VARIATION_PAIR_DTYPE.names == ("candidate", "variant", "info", "weight")
    assert va.VARIATION_UNDEFINED == 0xFFFFFFFF and va.VARIANT_OTHER == 4 and va.VARIATION_ZONES == ("none", "distal", "seed", "pam")
    by, silent, cost, largest = va.unpack_variation_row(np.array([[1 | 2 << 8 | 255 << 16 | 4 << 24, 5, 6, 7], [0xFFFFFFFF] * 4], dtype=np.uint32))
    assert by.tolist() == [[1, 2, 255, 4], [255] * 4] and silent.tolist() == [5, 0xFFFFFFFF] and cost.tolist() == [6, 0xFFFFFFFF] and largest[0] == 7
    first, touched, top, sil = va.unpack_variation_info(np.array([22 | 1 << 8 | 3 << 16, 0 | 32 << 8 | 2 << 16, 20 | 1 << 8 | 1 << 18], dtype=np.uint32))
    assert first.tolist() == [22, 0, 20] and touched.tolist() == [1, 32, 1] and top.tolist() == [3, 2, 0] and sil.tolist() == [0, 0, 1]
    header = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()
    assert "#define VSC_ABI_VERSION 5" in header and "#define VSC_VARIATION_UNDEFINED 0xFFFFFFFFu" in header


def test_pick_inputs_against_a_key_made_by_hand():
    loci = ed.locus_array([(0, 10, 0), (0, 11, 1), (1, 5, 0), (1, 9, 1)])
    pairs = np.zeros(6, dtype=va.VARIATION_PAIR_DTYPE)
    #                candidate, variant, first | touched << 8 | top << 16 | silent << 18, weight
    for k, row in enumerate([(0, 2, 21 | 1 << 8 | 3 << 16, 5), (0, 3, 3 | 1 << 8 | 1 << 16, 5), (2, 2, 12 | 2 << 8 | 2 << 16, 5),
                             (3, 0, 22 | 1 << 8 | 3 << 16 | 1 << 18, 5), (3, 3, 20 | 1 << 8 | 0 << 16, 5), (3, 4, 0 | 23 << 8 | 3 << 16, 5)]):
        pairs[k] = row
    got_loci, target, key, index = va.variation_pick_inputs(pairs, loci)
    assert index.tolist() == [0, 2, 5]  # disrupting, top seed or PAM: the distal pair, the silent pair and the N pair are left out
    assert got_loci.tobytes() == loci[[0, 2, 3]].tobytes() and target.dtype == np.uint32 and target.tolist() == [2, 2, 4]
    assert key.dtype == np.uint64 and key.tolist() == [3, 2, 3]  # PAM before seed
    spec = np.array([700, 9999, 5, 20000], dtype=np.uint64)
    _, _, key, _ = va.variation_pick_inputs(pairs, loci, extra_columns=[(spec, 14)])
    assert key.tolist() == [3 << 14 | 700, 2 << 14 | 5, 3 << 14 | 16383]
    assert va.variation_pick_inputs(pairs, loci, zones=(1,))[3].tolist() == [1] and va.variation_pick_inputs(pairs, loci, zones=(0, 1, 2, 3))[3].tolist() == [0, 1, 2, 4, 5]
    assert va.variation_pick_inputs(pairs[:0], loci)[2].shape == (0,)
    with pytest.raises(ValueError):
        va.variation_pick_inputs(pairs, loci, extra_columns=[(spec[:3], 14)])


def test_python_filters_need_the_shape():
    f = va.Genome._variation_args
    rows = [(1, 2, "A", "C"), (0, 3, "A", "G")]
    assert f(None, None, None, None, None, 23) is None
    shape, var, order, inverse, filt = f("SpCas9", rows, None, None, None, 23)
    assert shape is va.VARIATION_SHAPES["SpCas9"] and var["pos"].tolist() == [3, 2] and order.tolist() == [1, 0] and filt is None
    filt = f("SpCas9", rows, 9, (1, 2, 3, 255), ("pam", 2), 23)[4]
    assert (filt.max_cost, filt.max_by_zone, filt.require_zones, filt.reserved) == (9, 1 | 2 << 8 | 3 << 16 | 255 << 24, 12, 0)
    filt = f("SpCas9", rows, None, None, (), 23)[4]
    assert (filt.max_cost, filt.max_by_zone, filt.require_zones) == (0xFFFFFFFF, 0xFFFFFFFF, 0)
    already = va.site_variants(rows)[0]
    assert f("SpCas9", already, None, None, None, 23)[1] is not None and f("SpCas9", already, None, None, None, 23)[2] is None
    for bad in ((None, rows, None, None, None), (None, None, 1, None, None), (None, None, None, (0, 0, 0, 0), None), (None, None, None, None, (3,)),
                ("SpCas9", None, None, None, None), ("Cas9", rows, None, None, None), (7, rows, None, None, None), ("Cas12a", rows, None, None, None),
                ("SpCas9", rows, -1, None, None), ("SpCas9", rows, None, (1, 2, 3), None), ("SpCas9", rows, None, (1, 2, 3, 256), None),
                ("SpCas9", rows, None, None, (4,)), ("SpCas9", rows, None, None, ("tail",))):
        with pytest.raises(ValueError):
            f(*bad, 23)


def test_every_validation_error_of_the_host_entry():
    L = va.lib()
    contigs = ed.small_genome()
    ct = vc.contig_array(contigs)
    loci = ed.locus_array([(ed.MAIN, 100, 0), (ed.MAIN, 99, 1)])
    ok = va.VARIATION_SHAPES["SpCas9"]._struct()
    rows = np.full((2, 4), 9, dtype=np.uint32)
    count = C.c_uint64(77)

    def call(shape=ok, variants=None, n_v=None, lo=loci, n=2, contig_table=ct, n_contigs=len(ct)):
        return L.vsc_variation_host(_lib.ptr(contig_table), n_contigs, _lib.ptr(lo), n, C.byref(shape) if shape is not None else None,
                                    _lib.ptr(variants), len(variants) if n_v is None and variants is not None else (n_v or 0), _lib.ptr(rows), None, 0,
                                    C.byref(count), None)

    def raw(records):
        out = np.zeros(len(records), dtype=va.VARIANT_DTYPE)
        for k, r in enumerate(records):
            out[k] = r
        return out

    other = 4 << 16
    assert call(variants=raw([(ed.MAIN, 100, 1 | other, 1), (ed.MAIN, 100, 1 | 2 << 16, 2)])) == 0 and not (rows == 9).any() and count.value == 4
    rows[:] = 9
    count.value = 77
    last = len(contigs[ed.MAIN]) - 1
    for bad in ([(ed.MAIN, 6, 1 | other, 0), (ed.MAIN, 5, 1 | other, 0)],  # out of order inside a contig
                [(ed.MAIN, 0, 1 | other, 0), (0, 5, 1 | other, 0)],        # ... and across contigs
                [(len(contigs), 0, 1 | other, 0)], [(0xFFFFFFFF, 0, 1 | other, 0)],  # an unknown contig
                [(ed.MAIN, 5, 0 | other, 0)],                               # a span of 0
                [(ed.MAIN, last, 2 | other, 0)], [(ed.MAIN, last + 1, 1 | other, 0)], [(0, 0, 23 | other, 0)], [(ed.MAIN, 0xFFFFFFFF, 1 | other, 0)],  # beyond its contig
                [(ed.MAIN, 5, 2 | 0 << 16, 0)], [(ed.MAIN, 5, 65535 | 3 << 16, 0)],  # alt 0..3 with span != 1
                [(ed.MAIN, 5, 1 | 5 << 16, 0)], [(ed.MAIN, 5, 1 | 7 << 16, 0)], [(ed.MAIN, 5, 1 | other | 1 << 19, 0)], [(ed.MAIN, 5, 1 | 1 << 31, 0)],  # alt > 4, other bits
                [(ed.MAIN, 5, 1 | other, 0xFFFFFFFF)]):                     # a weight of 0xFFFFFFFF
        assert call(variants=raw(bad)) == -22, bad
    for kw in (dict(site_len=15), dict(site_len=33), dict(site_len=0xFFFFFFFF), dict(zones=1 << 46), dict(accept=(0, 1 << 28)), dict(site_len=16, accept=(0, 1)),
               dict(site_len=31, zones=1 << 62)):  # a bad shape
        assert call(shape=va.VariationShape(validate=False, **kw)._struct()) == -22, kw
    for field in ("reserved0", 0, 1, 2, 3):  # a reserved field
        st = va.VARIATION_SHAPES["SpCas9"]._struct()
        if field == "reserved0":
            st.reserved0 = 1
        else:
            st.reserved[field] = 1
        assert call(shape=st) == -22
    good = raw([(ed.MAIN, 100, 1 | other, 1)])
    assert call(shape=None) == -22 and call(variants=None, n_v=3) == -22 and call(lo=None) == -22 and call(contig_table=None) == -22  # NULL arguments
    assert call(variants=good, n=0xFFFFFFFF) == -34 and call(variants=good, n_v=0xFFFFFFFF) == -34  # n, n_v above 0xFFFFFFFE
    assert (rows == 9).all() and count.value == 77  # every refusal comes before anything is written
    # what the bounds allow: the first and the last base, a whole contig, the largest weight, ties
    edge = raw([(0, 0, 22 | other, 0xFFFFFFFE), (ed.MAIN, 0, 1 | 0 << 16, 0), (ed.MAIN, 0, 1 | 3 << 16, 0), (ed.MAIN, last, 1 | other, 0)])
    assert call(variants=edge) == 0
    assert call(variants=None, n=0) == 0 and call(variants=good, lo=None, n=0) == 0  # n == 0: nothing to do
    # the capacity contract
    pairs = np.full(8, 0x5A5A5A5A, dtype=np.uint32).view(va.VARIATION_PAIR_DTYPE)
    cov = np.full((1, 2), 7, dtype=np.uint32)
    rc = L.vsc_variation_host(_lib.ptr(ct), len(ct), _lib.ptr(loci), 2, C.byref(ok), _lib.ptr(good), 1, _lib.ptr(rows), _lib.ptr(pairs), 1, C.byref(count),
                              _lib.ptr(cov))
    assert rc == -34 and count.value == 2 and (pairs.view(np.uint32) == 0x5A5A5A5A).all() and cov.tolist() == [[2, 0]] and rows[0, 2] == 1
    rc = L.vsc_variation_host(_lib.ptr(ct), len(ct), _lib.ptr(loci), 2, C.byref(ok), _lib.ptr(good), 1, None, _lib.ptr(pairs), 2, None, None)
    assert rc == 0 and pairs["candidate"].tolist() == [0, 1] and pairs["variant"].tolist() == [0, 0] and pairs["weight"].tolist() == [1, 1]
    assert pairs["info"].tolist() == [0 | 1 << 8 | 1 << 16, 21 | 1 << 8 | 3 << 16]  # read position 0 on the + site at 100; 22 - (100 - 99) = 21 on the - site at 99: the PAM


def test_the_stand_alone_check_builds_and_runs_clean(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "variation_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.join(ROOT, "varscot_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                            "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "variation_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.startswith("ok: ") and "runtime error" not in run.stderr and "ERROR" not in run.stderr, \
        (run.returncode, run.stdout, run.stderr)

"""The variant map on the host (vsc_variant_map_*, no device): every window position of the scenario against the merger's
getSnpType, the shadow regions against filterRefAlignment's predicate, the empty map and the refused arguments."""
import ctypes as C

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import variants_cases as vc
from oracle import merge_oracle as mo

UNKNOWN = 0xFFFFFFFF


def _map_of(sc, windows, tmp_path, vcf, sample):
    """(reference PackedGenome, window PackedGenome built by the library, VariantMap); the library's windows are the oracle's."""
    ref = va.PackedGenome.from_sequences(sc.seqs, sc.names)
    (tmp_path / "in.vcf").write_text(vcf)
    win = va.variant_windows(ref, tmp_path / "in.vcf", sample=sample, threads=2)
    assert list(win.names) == [w[0] for w in windows]
    assert [int(x) for x in win.contigs["length"]] == [len(w[1]) for w in windows]
    return ref, win, va.VariantMap(win, ref)


@pytest.mark.parametrize("which,sample", [("vcf", 0), ("vcf", 1), ("vcf_wrapped", 0)])
def test_locate_and_tag_equal_get_snp_type(tmp_path, which, sample):
    sc = vc.scenario(vc.SEEDS[0])
    windows = sc.windows(sample, which)
    _, _, vmap = _map_of(sc, windows, tmp_path, getattr(sc, which), sample)
    info = vmap.info()
    assert info["windows"] == len(windows)
    assert info["unknown_chr"] == sum(1 for w in windows if w[0].split("_")[0] not in sc.chroms) >= vc.FLOORS["chrun_windows"]
    if which == "vcf_wrapped":
        assert any(mo.c_atoi(w[0].split("_")[1]) < 0 for w in windows)  # the start that wrapped
    seen_var = seen_shift = seen_multi = 0
    for w, (wid, seq) in enumerate(windows):
        fid = wid.split("_")
        contig = sc.chroms.index(fid[0]) if fid[0] in sc.chroms else UNKNOWN
        for pos in range(len(seq) - 23 + 1):
            pos1 = (pos + mo.c_atoi(fid[1])) % (1 << 32)
            pot = mo.Pot("g", fid[0], pos1, "+", "", [-1])
            mo.get_snp_type(pot, fid, 23)
            lab = vmap.locate(w, pos)
            n_var = 0 if pot.snp_type == "REF" else pot.snp_type.count(",") + 1
            assert (int(lab["contig"]), int(lab["pos"]), int(lab["n_var"]), int(lab["flags"])) == (contig, pot.pos, n_var, 1 if n_var else 0), (wid, pos)
            assert vmap.tag(w, pos) == pot.snp_type, (wid, pos)
            seen_var += n_var > 0
            seen_multi += n_var > 1
            seen_shift += pot.pos != pos1
    assert seen_var and seen_multi and seen_shift
    vmap.close()


@pytest.mark.parametrize("which,sample", [("vcf", 1), ("vcf_wrapped", 0)])
def test_shadow_equals_filter_ref_alignment(tmp_path, which, sample):
    sc = vc.scenario(vc.SEEDS[0])
    windows = sc.windows(sample, which)
    _, _, vmap = _map_of(sc, windows, tmp_path, getattr(sc, which), sample)
    regions = vmap.shadow()
    assert regions.info()["rule"] == _lib.REGION_INSIDE
    info = [w[0].split("_") + [str(len(w[1]))] for w in windows]
    inside = 0
    for c, seq in enumerate(sc.seqs):
        # the predicate per position, from the windows of this chromosome once (vc.shadows is the loop of the merger)
        mine = [(mo.c_atoi(w[1]) % (1 << 32), (mo.c_atoi(w[1]) + mo.c_atoi(w[-1])) % (1 << 32)) for w in info if w[0] == sc.chroms[c]]
        for pos in range(len(seq) - 23 + 1):
            want = any(pos >= s and pos + 23 <= e for s, e in mine)
            assert regions.contains(c, pos) == want, (c, pos)
            inside += want
        for pos in range(0, len(seq) - 23 + 1, 97):  # and the merger's own loop on a sample of them
            assert regions.contains(c, pos) == vc.shadows(info, sc.chroms[c], pos)
    assert inside > 1000
    regions.close()
    vmap.close()


def test_empty_map_and_sample_without_alt_allele(tmp_path):
    sc = vc.scenario(vc.SEEDS[0])
    assert sc.windows(0, "vcf_no_alt") == []
    _, win, vmap = _map_of(sc, [], tmp_path, sc.vcf_no_alt, 0)
    assert len(win.contigs) == 0
    assert vmap.info() == {"windows": 0, "variants": 0, "unknown_chr": 0, "max_variants": 0}
    regions = vmap.shadow()
    assert regions.info()["intervals"] == 0 and not regions.contains(0, 100)
    with pytest.raises(va.VarscotError) as e:
        vmap.locate(0, 0)
    assert e.value.code == -22
    with pytest.raises(va.VarscotError):
        vmap.tag(0, 0)


def test_ids_the_reference_would_split_differently():
    """No '_' at all, a non-numeric start, a triple cut short, a chromosome the reference does not have."""
    ref = va.PackedGenome.from_sequences(["ACGT" * 50, "GGCA" * 50], names=["chr1 first", "chrUn_x second"])
    ids = ["chr1_10_ALT_15_A_C_20_AT_A", "chrUn_x_5_ALT_9_A_ACG", "chr1_-3_REF", "chr9", "chr1_7_ALT_12_A"]
    win = type("W", (), {"names": ids, "contigs": np.zeros(len(ids), dtype=va.CONTIG_DTYPE)})()
    win.contigs["length"] = [60, 50, 40, 30, 45]
    vmap = va.VariantMap(win, ref)
    assert vmap.info() == {"windows": 5, "variants": 3, "unknown_chr": 2, "max_variants": 2}
    for w, wid in enumerate(ids):
        fid = wid.split("_")
        for pos in range(0, 30):
            pot = mo.Pot("g", fid[0], (pos + mo.c_atoi(fid[1] if len(fid) > 1 else "0")) % (1 << 32), "+", "", [-1])
            mo.get_snp_type(pot, fid, 23)
            lab = vmap.locate(w, pos)
            assert int(lab["pos"]) == pot.pos and vmap.tag(w, pos) == pot.snp_type, (wid, pos)
            assert int(lab["contig"]) == (0 if fid[0] == "chr1" else UNKNOWN)
    shadow = vmap.shadow()  # chr1 [10, 70) and [7, 52): the negative start and the unknown chromosomes shadow nothing
    assert shadow.info()["intervals"] == 2
    assert [shadow.contains(0, p) for p in (6, 7, 29, 30, 47, 48)] == [False, True, True, True, True, False]
    assert not shadow.contains(1, 5)


def test_invalid_arguments():
    L = va.lib()
    ref = va.PackedGenome.from_sequences(["ACGT" * 50], names=["chr1"])
    names = (C.c_char_p * 1)(b"chr1")
    pool = np.frombuffer(b"chr1_3_REF\n", dtype=np.uint8).copy()
    off = np.array([0, len(pool)], dtype=np.uint64)
    wc = np.zeros(1, dtype=va.CONTIG_DTYPE)
    wc["length"] = 45
    h = C.c_void_p()
    ptr = _lib.ptr
    assert L.vsc_variant_map_build(ptr(pool), ptr(off), ptr(wc), 1, ptr(ref.contigs), names, 1, None) == -22
    assert L.vsc_variant_map_build(None, ptr(off), ptr(wc), 1, ptr(ref.contigs), names, 1, C.byref(h)) == -22 and not h.value
    assert L.vsc_variant_map_build(ptr(pool), None, ptr(wc), 1, ptr(ref.contigs), names, 1, C.byref(h)) == -22
    assert L.vsc_variant_map_build(ptr(pool), ptr(off), None, 1, ptr(ref.contigs), names, 1, C.byref(h)) == -22
    assert L.vsc_variant_map_build(ptr(pool), ptr(off), ptr(wc), 1, None, names, 1, C.byref(h)) == -22
    bad = np.array([5, 5], dtype=np.uint64)  # no room for an id and its separator
    assert L.vsc_variant_map_build(ptr(pool), ptr(bad), ptr(wc), 1, ptr(ref.contigs), names, 1, C.byref(h)) == -22
    assert L.vsc_variant_map_build(ptr(pool), ptr(off), ptr(wc), 1, ptr(ref.contigs), names, 1, C.byref(h)) == 0 and h.value
    st = _lib.VariantMapStats()
    assert L.vsc_variant_map_info(None, C.byref(st)) == -22 and L.vsc_variant_map_info(h, None) == -22
    lab = np.zeros(1, dtype=va.VARIANT_LABEL_DTYPE)
    assert L.vsc_variant_map_locate(h, 1, 0, ptr(lab)) == -22 and L.vsc_variant_map_locate(h, 0, 0, None) == -22
    assert L.vsc_variant_map_locate(None, 0, 0, ptr(lab)) == -22
    assert L.vsc_variant_map_locate(h, 0, 4, ptr(lab)) == 0 and tuple(lab[0]) == (0, 7, 0, 0)
    buf = C.create_string_buffer(3)
    assert L.vsc_variant_map_tag(h, 0, 0, buf, 3) == 3 and buf.value == b"RE"  # cut at len - 1, the full length returned
    assert L.vsc_variant_map_tag(h, 1, 0, buf, 3) == -22 and L.vsc_variant_map_tag(h, 0, 0, None, 3) == -22
    r = C.c_void_p()
    assert L.vsc_variant_map_shadow(None, C.byref(r)) == -22 and L.vsc_variant_map_shadow(h, None) == -22
    L.vsc_variant_map_free(h)
    L.vsc_variant_map_free(None)
    # calls that need the device refuse null arguments before they touch it
    assert L.vsc_hits_variants(None, None, None, None, 0, None) == -22
    assert L.vsc_search_summary_variants(None, None, None, None, 0, None, None, 0, None, None, None) == -22


def test_individual_rows_adds_the_two_sides():
    a, b, w = (np.zeros(2, dtype=va.SUMMARY_DTYPE) for _ in range(3))
    a["nm"][:, 1], a["mit_sum"], a["mit_ub"], a["on_target"] = [5, 7], [100, 200], [1, 0], [1, 0]
    b["nm"][:, 1], b["mit_sum"] = [2, 7], [40, 200]
    w["nm"][:, 1], w["nm"][:, 2], w["mit_sum"], w["on_target"] = [1, 0], [0, 3], [9, 30], [0, 1]
    got = va.individual_rows(a, b, w)
    assert got["nm"][:, 1].tolist() == [4, 0] and got["nm"][:, 2].tolist() == [0, 3]
    assert got["mit_sum"].tolist() == [69, 30] and got["mit_ub"].tolist() == [1, 0] and got["on_target"].tolist() == [1, 1]

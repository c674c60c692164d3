"""The variant map for sites of any length on the host (vsc_variant_map_locate_len / _tag_len / _shadows, no device): every
window position of every shape of tests/pattern_variants_cases.py against the merger's getSnpType with seq_len = L, every
reference position against filterRefAlignment's predicate, len = 23 against the calls for the 23-base read, a wrapped window
start, the refused arguments - and the floors of the scenario, counted on the oracle's own output."""
import ctypes as C

import numpy as np
import pytest

import varscot_amd as va
from varscot_amd import _lib
import pattern_variants_cases as pv
import variants_cases as vc
from oracle import merge_oracle as mo

UNKNOWN = 0xFFFFFFFF
SHAPES = list(pv.SHAPES)


def _map_of(sc, windows, tmp_path, vcf, sample, seq_len):
    """(reference PackedGenome, window PackedGenome built by the library, VariantMap); the library's windows are the oracle's."""
    ref = va.PackedGenome.from_sequences(sc.seqs, sc.names)
    (tmp_path / "in.vcf").write_text(vcf)
    win = va.variant_windows(ref, tmp_path / "in.vcf", sample=sample, seq_len=seq_len, threads=2)
    assert list(win.names) == [w[0] for w in windows]
    assert [int(x) for x in win.contigs["length"]] == [len(w[1]) for w in windows]
    return ref, win, va.VariantMap(win, ref)


@pytest.mark.parametrize("shape", SHAPES)
def test_floors_of_the_scenario(shape):
    fl = pv.scenario(shape).case().floors()
    assert all(fl[k] >= v for k, v in pv.FLOORS.items()), fl


@pytest.mark.parametrize("shape,which", [(s, "vcf") for s in SHAPES] + [("sa", "vcf_wrapped")])
def test_locate_len_and_tag_len_equal_get_snp_type(tmp_path, shape, which):
    sc = pv.scenario(shape)
    L = sc.L
    windows = sc.windows(0, which)
    _, _, vmap = _map_of(sc, windows, tmp_path, getattr(sc, which), 0, L)
    if which == "vcf_wrapped":
        assert any(mo.c_atoi(w[0].split("_")[1]) < 0 for w in windows)  # the start that wrapped
    seen_var = seen_shift = seen_multi = 0
    for w, (wid, seq) in enumerate(windows):
        fid = wid.split("_")
        contig = sc.chroms.index(fid[0]) if fid[0] in sc.chroms else UNKNOWN
        for pos in range(len(seq) - L + 1):
            pos2, tag, moved = pv.walk(fid, pos, L)
            lab = vmap.locate(w, pos, L)
            n_var = pv.n_var_of(tag)
            assert (int(lab["contig"]), int(lab["pos"]), int(lab["n_var"]), int(lab["flags"])) == (contig, pos2, n_var, 1 if n_var else 0), (wid, pos)
            assert vmap.tag(w, pos, L) == tag, (wid, pos)
            seen_var += n_var > 0
            seen_multi += n_var > 1
            seen_shift += moved
    assert seen_var and seen_multi and seen_shift
    vmap.close()


def test_length_23_gives_the_existing_calls_answers(tmp_path):
    sc = vc.scenario(vc.SEEDS[0])
    windows = sc.windows(0)
    _, _, vmap = _map_of(sc, windows, tmp_path, sc.vcf, 0, 23)
    L = va.lib()
    a, b = np.zeros(1, dtype=_lib.VARIANT_LABEL_DTYPE), np.zeros(1, dtype=_lib.VARIANT_LABEL_DTYPE)
    for w, (_, seq) in enumerate(windows):
        for pos in range(len(seq)):
            assert L.vsc_variant_map_locate(vmap._h, w, pos, _lib.ptr(a)) == 0 == L.vsc_variant_map_locate_len(vmap._h, w, pos, 23, _lib.ptr(b))
            assert a.tobytes() == b.tobytes(), (w, pos)
            n = int(L.vsc_variant_map_tag_len(vmap._h, w, pos, 23, None, 0))
            buf = C.create_string_buffer(n + 1)
            assert L.vsc_variant_map_tag_len(vmap._h, w, pos, 23, buf, n + 1) == n
            assert buf.value.decode() == vmap.tag(w, pos)
    vmap.close()


@pytest.mark.parametrize("shape,which", [(s, "vcf") for s in SHAPES] + [("sa", "vcf_wrapped")])
def test_shadows_equals_filter_ref_alignment(tmp_path, shape, which):
    sc = pv.scenario(shape)
    L = sc.L
    windows = sc.windows(0, which)
    _, _, vmap = _map_of(sc, windows, tmp_path, getattr(sc, which), 0, L)
    info = [w[0].split("_") + [str(len(w[1]))] for w in windows]
    inside = 0
    for c, seq in enumerate(sc.seqs):
        # the predicate per position, from the windows of this chromosome once (vc.shadows is the loop of the merger)
        mine = [(mo.c_atoi(w[1]) % (1 << 32), (mo.c_atoi(w[1]) + mo.c_atoi(w[-1])) % (1 << 32)) for w in info if w[0] == sc.chroms[c]]
        want = np.zeros(len(seq), dtype=bool)
        pos = np.arange(len(seq), dtype=np.int64)
        for s, e in mine:
            want |= (pos >= s) & (pos + L <= e)
        want[len(seq) - L + 1:] = False  # (no site of L bases starts there)
        got = np.array([vmap.shadows(c, p, L) for p in range(len(seq))])
        assert np.array_equal(got, want), (c, np.flatnonzero(got != want)[:5])
        inside += int(want.sum())
        for p in range(0, len(seq) - L + 1, 97):  # and the merger's own loop on a sample of them
            assert bool(got[p]) == vc.shadows(info, sc.chroms[c], p, L)
    assert inside > 1000
    vmap.close()


def test_refused_arguments(tmp_path):
    sc = pv.scenario("sa")
    windows = sc.windows(0)
    _, _, vmap = _map_of(sc, windows, tmp_path, sc.vcf, 0, sc.L)
    L = va.lib()
    lab = np.zeros(1, dtype=_lib.VARIANT_LABEL_DTYPE)
    buf = C.create_string_buffer(64)
    n = len(windows)
    for bad_len in (0, 15, 33, 1 << 31):
        assert L.vsc_variant_map_locate_len(vmap._h, 0, 0, bad_len, _lib.ptr(lab)) == -22
        assert L.vsc_variant_map_tag_len(vmap._h, 0, 0, bad_len, buf, 64) == -22
        assert L.vsc_variant_map_shadows(vmap._h, 0, 0, bad_len) == -22
    for good_len in (16, 32):
        assert L.vsc_variant_map_locate_len(vmap._h, 0, 0, good_len, _lib.ptr(lab)) == 0
        assert L.vsc_variant_map_tag_len(vmap._h, 0, 0, good_len, buf, 64) > 0
        assert L.vsc_variant_map_shadows(vmap._h, 0, 0, good_len) in (0, 1)
    assert L.vsc_variant_map_locate_len(vmap._h, n, 0, 27, _lib.ptr(lab)) == -22       # a window the map does not have
    assert L.vsc_variant_map_tag_len(vmap._h, n, 0, 27, buf, 64) == -22
    assert L.vsc_variant_map_shadows(vmap._h, len(sc.seqs), 0, 27) == -22               # a contig the reference does not have
    assert L.vsc_variant_map_locate_len(None, 0, 0, 27, _lib.ptr(lab)) == -22           # null arguments
    assert L.vsc_variant_map_locate_len(vmap._h, 0, 0, 27, None) == -22
    assert L.vsc_variant_map_tag_len(None, 0, 0, 27, buf, 64) == -22
    assert L.vsc_variant_map_tag_len(vmap._h, 0, 0, 27, None, 64) == -22
    assert L.vsc_variant_map_shadows(None, 0, 0, 27) == -22
    with pytest.raises(va.VarscotError) as e:
        vmap.shadows(0, 0, 40)
    assert e.value.code == -22
    assert vmap.shadows(0, len(sc.seqs[0]) - 5, 27) is False  # beyond the contig's last site: not an error
    vmap.close()


def test_pattern_search_refuses_what_v_does_not_combine_with(tmp_path):
    """The tool's argument checks come before the index and the device: -v with -u / -U / -Z / -w / -T / -K / -S, -v without
    -O, -n without -v and a -v file that is no .vcf end with a usage error; with -v the message names it."""
    import os
    import subprocess
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "varscot_amd", "bin", "pattern_search")
    base = [tool, "-i", str(tmp_path / "idx"), "-q", pv.SHAPES["sa"], "-R", str(tmp_path / "guides.fa"), "-M", "4"]
    out, vcf = ["-O", str(tmp_path / "o.tsv")], ["-v", str(tmp_path / "in.vcf")]
    run = lambda args: subprocess.run(args, capture_output=True, text=True, timeout=60)
    for extra in (["-u", "1,1", "-p", "0,21"], ["-u", "1,1", "-p", "0,21", "-U", str(tmp_path / "u.tsv")],
                  ["-u", "1,1", "-p", "0,21", "-Z", str(tmp_path / "z.tsv")],
                  ["-u", "1,1", "-p", "0,21", "-Z", str(tmp_path / "z.tsv"), "-W", str(tmp_path / "t.tsv"), "-w", str(tmp_path / "w.tsv")],
                  ["-T", str(tmp_path / "h.tsv")], ["-W", str(tmp_path / "t.tsv"), "-K", "3"], ["-W", str(tmp_path / "t.tsv"), "-S", "0.5"]):
        r = run(base + out + vcf + extra)
        assert r.returncode == 1 and "-v" in r.stderr, (extra, r.stderr)
    r = run(base + vcf)  # no -O
    assert r.returncode == 1 and "-v" in r.stderr
    assert run(base + out + ["-n", "1"]).returncode == 1
    r = run(base + out + ["-v", str(tmp_path / "in.txt")])
    assert r.returncode == 1 and "-v" in r.stderr
    r = run(base + out + vcf + ["-n", "x"])
    assert r.returncode == 1 and "-n" in r.stderr

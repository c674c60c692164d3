"""The variation join beyond one launch (vsc_loci_variation, vsc_guides_filter_variation): more candidates than a launch has lanes
and more tiles than it has waves, sized from the device's CU count as tests/test_wide.py sizes its launches; against the
restatement of tests/variation_cases.py, repeated."""
import ctypes as C

import numpy as np
import pytest
import torch

import edit_cases as ed
import variation_cases as vc
import varscot_amd as va
import wide_cases as wc
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

TILE = 1024  # candidates per wave of the pairs' and the filter's passes


def launch_waves():
    """The waves of a launch capped as the rows kernel's grid is: CUs x 8 workgroups of 4 waves."""
    return torch.cuda.get_device_properties(0).multi_processor_count * wc.GROUPS_PER_CU * wc.WAVES_PER_GROUP


def test_more_candidates_than_a_launch_has_lanes_and_more_tiles_than_waves():
    ctx = va.Context(0)
    shape = vc.spcas9()
    contigs = vc.wide_genome(23)
    gen = ctx.load_genome(va.PackedGenome.from_sequences(list(contigs)))
    variants, where = vc.variant_sets(contigs, 23)["ends"]  # several pairs per candidate: runs of them cross tile boundaries
    base_loci = vc.loci_of(contigs, where) + ed.invalid_loci(contigs)
    base = vc.expected(contigs, base_loci, shape, variants)
    sh, var, arr = vc.shape_of(shape), vc.variant_array(variants), ed.locus_array(base_loci)
    m = len(base_loci)
    n = (launch_waves() + 3) * TILE + 17
    assert n > 3 * m and n > launch_waves() * 64
    idx = np.arange(n) % m
    loci = arr[idx]
    rows, pairs, coverage, stats = gen.variation(loci, sh, var, coverage=True)
    assert rows.tobytes() == base["rows"][idx].tobytes()
    reps, rem = divmod(n, m)
    bp = base["pairs"]
    parts = []
    for k in range(reps + 1):
        part = (bp if k < reps else bp[bp["candidate"] < rem]).copy()
        part["candidate"] += np.uint32(k * m)
        parts.append(part)
    want_pairs = np.concatenate(parts)
    assert len(want_pairs) > 3 * TILE and np.bincount(bp["candidate"]).max() >= 3
    assert stats["pairs"] == len(want_pairs) == len(pairs) and pairs.tobytes() == want_pairs.tobytes()
    last = np.zeros_like(base["coverage"])
    tail = bp[bp["candidate"] < rem]
    np.add.at(last, (tail["variant"].astype(np.int64), (tail["info"] >> 18 & 1).astype(np.int64)), 1)
    assert (coverage == reps * base["coverage"] + last).all()
    assert sum(stats[k] for k in vc.CLASSES) == n and stats["variants_covered"] == base["stats"]["variants_covered"]
    # the filter over the same tiles: the survivors in input order
    keep = np.array([vc.keep(z, c, max_cost=30, max_by_zone=(255, 255, 255, 1)) for z, c in zip(base["by_zone"], base["cost"])])
    assert 0 < keep.sum() < len(keep)
    codes = np.arange(n, dtype=np.uint64) * np.uint64(3)
    L = va.lib()
    h, out = C.c_void_p(), C.c_void_p()
    _lib.check(L.vsc_debug_guides_from_host(ctx._h, _lib.ptr(codes), _lib.ptr(loci), n, C.byref(h)), ctx._h)
    f = _lib.VariationFilterStruct(30, 255 | 255 << 8 | 255 << 16 | 1 << 24, 0, 0)
    st = sh._struct()
    _lib.check(L.vsc_guides_filter_variation(ctx._h, gen._h, h, C.byref(st), _lib.ptr(var), len(var), C.byref(f), C.byref(out)), ctx._h)
    k = int(L.vsc_guides_count(out))
    pc, pl = C.c_void_p(), C.c_void_p()
    _lib.check(L.vsc_guides_data(out, C.byref(pc), C.byref(pl)), ctx._h)
    got_codes = np.frombuffer((C.c_char * (k * 8)).from_address(pc.value), dtype=np.uint64)
    got_loci = np.frombuffer((C.c_char * (k * 16)).from_address(pl.value), dtype=va.LOCUS_DTYPE)
    chosen = np.nonzero(keep[idx])[0]
    assert got_codes.tobytes() == codes[chosen].tobytes() and got_loci.tobytes() == loci[chosen].tobytes()
    L.vsc_guides_free(out)
    L.vsc_guides_free(h)
    gen.close()
    ctx.close()

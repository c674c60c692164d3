"""HDR knock-in design over candidate guides (vsc_guides_hdr, vsc_guides_filter_hdr) on the synthetic hg38-sized genome of
varscot_amd.synth, one GPU, beside the enumeration that produces the candidates and the prime-editing rows kernel - the same
context width, the same join and the same launch shape - over the same candidates and edits, in one run and one process
(prime_bench's genome, candidates and edit sets).

    python tools/hdr_bench.py                      JSON to profiles/hdr.json (and stdout)
    python tools/hdr_bench.py --calls 1 --warmup 1 (what a kernel trace needs: run it under rocprofv3 --kernel-trace --stats)

Steps (each under its own time limit, --step-seconds: W warm-up calls, then K timed calls, fastest .. slowest)
  enumerate    vsc_guides_enumerate alone: NGG, both strands, no filter, no regions - a yardstick; kernels' time =
               vsc_timing.scan_ms (count pass + scan, write pass)
  prime_none / prime_snv / prime_exons   vsc_guides_prime under the PE2 preset without edits, with about 10^6 random SNVs and with
               an SNV at every fourth position of the 250 000 exon-like intervals: prime_rows_kernel = vsc_timing.score_ms - the
               other yardstick
  rows_none / rows_snv / rows_exons      vsc_guides_hdr under the SpCas9 preset over the same three edit sets, pairs counted only:
               hdr_rows_kernel = vsc_timing.score_ms, the pairs' count pass + scan + write pass (coverage and pairs by flag) =
               vsc_timing.scan_ms; each without a CDS and with the exon-like intervals as a CDS (every interval a transcript)
  pairs_snv    the random SNVs with the CDS, the pairs written and copied to the host
  filter       vsc_guides_filter_hdr, the random SNVs, the CDS: both passes and the scan = vsc_timing.score_ms
Reported beside each kernel time, the floor DERIVED from the shapes: 24 bytes per candidate (16 of locus read, 8 of
row written) for the rows kernel at the 6.3 TB/s a float4 copy kernel reaches."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import varscot_amd as va  # noqa: E402
from varscot_amd import _lib, dist as vdist, synth  # noqa: E402
from varscot_amd.api import _enum_params  # noqa: E402
from edit_bench import targets_of_global  # noqa: E402
from effects_bench import Table, exon_segments  # noqa: E402
from efficiency_bench import FLOAT4_COPY_TBS, enumerate_once  # noqa: E402
from microhomology_bench import step_limit  # noqa: E402
from prime_bench import snvs_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--random-edits", type=int, default=1_000_000)
    ap.add_argument("--intervals", type=int, default=250_000)
    ap.add_argument("--fraction", type=float, default=0.03)
    ap.add_argument("--exon-step", type=int, default=4)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdr.json"))
    args = ap.parse_args()
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    print(json.dumps({"planes_words": int(len(hi))}), flush=True)
    rng = np.random.default_rng(30)
    random_edits = snvs_of(targets_of_global(table, np.unique(rng.integers(0, span, size=args.random_edits, dtype=np.int64))), rng)
    iv = synth.synthetic_regions(table, args.intervals, args.fraction)
    start = np.asarray(table["offset"], dtype=np.int64)[iv["contig"]] + iv["start"].astype(np.int64)
    length = (iv["end"].astype(np.int64) - iv["start"].astype(np.int64))
    g = np.repeat(start - np.concatenate(([0], np.cumsum(length)[:-1])), length) + np.arange(int(length.sum()), dtype=np.int64)
    g = np.unique(g)[::args.exon_step]
    exon_edits = snvs_of(targets_of_global(table, g), rng)
    del g
    exons = exon_segments(table, args.intervals, args.fraction)
    cds = va.Cds(Table(table), exons, n_tx=len(exons), sort=False)
    print(json.dumps({"random_edits": len(random_edits), "exon_edits": len(exon_edits), "segments": len(exons)}), flush=True)
    with step_limit("load", args.step_seconds):
        ctx = va.Context(0)
        genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    L = va.lib()
    params = _enum_params("GG", "both", (0, 0), 0, 0)
    res = {"genome_bases": args.bases, "calls": args.calls, "warmup": args.warmup, "float4_copy_tbs": FLOAT4_COPY_TBS,
           "random_edits": len(random_edits), "exon_edits": len(exon_edits), "segments": len(exons),
           "coding_bases": cds.info()["coding_bases"]}

    def report(key, value):
        res[key] = value
        print(json.dumps({key: value}), flush=True)
        with open(args.out, "w") as f:  # (what was measured before a step's limit ends the process is in the file)
            json.dump(res, f, indent=1)
            f.write("\n")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        return [fn() for _ in range(args.calls)]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with step_limit("enumerate", args.step_seconds):
        runs = timed(lambda: enumerate_once(ctx, genome, params))
        n = runs[0][2]
        report("enumerate", {"candidates": n, "kernels_ms": sorted(r[1] for r in runs), "wall_ms": sorted(r[0] for r in runs)})
        _, _, _, h = enumerate_once(ctx, genome, params, keep=True)
    enum_ms = res["enumerate"]["kernels_ms"][0]
    hbm_rows_ms = 24.0 * n / (FLOAT4_COPY_TBS * 1e12) * 1e3
    count = C.c_uint64()
    sets = (("none", None), ("snv", random_edits), ("exons", exon_edits))

    # the yardstick: prime_rows_kernel over the same candidates and edits
    pe2, pst = va.PRIME_EDITORS["PE2"]._struct(), _lib.PrimeStats()
    prime_ms = {}
    for key, edits in sets:
        with step_limit("prime_" + key, args.step_seconds):
            n_e = 0 if edits is None else len(edits)

            def prime_once():
                t0 = time.perf_counter()
                _lib.check(L.vsc_guides_prime(ctx._h, genome._h, h, C.byref(pe2), _lib.ptr(edits) if n_e else None, n_e, None, None, 0,
                                              C.byref(count), None, C.byref(pst)), ctx._h)
                return (time.perf_counter() - t0) * 1e3, ctx.timing()["score_ms"]

            runs = timed(prime_once)
            prime_ms[key] = sorted(r[1] for r in runs)
            report("prime_" + key, {"candidates": n, "edits": n_e, "pairs": int(pst.pairs), "rows_kernel_ms": prime_ms[key],
                                    "wall_ms": sorted(r[0] for r in runs)})

    shape, st = va.HDR_NUCLEASES["SpCas9"]._struct(), _lib.HdrStats()

    def hdr_step(name, key, edits, with_cds, write_pairs):
        with step_limit(name, args.step_seconds):
            n_e = 0 if edits is None else len(edits)
            ch = cds._h if with_cds else None
            pairs = None
            if write_pairs:
                _lib.check(L.vsc_guides_hdr(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(edits), n_e, ch, None, None, None, 0, C.byref(count),
                                            None, None), ctx._h)
                pairs = np.empty(int(count.value), dtype=va.HDR_PAIR_DTYPE)

            def once():
                t0 = time.perf_counter()
                _lib.check(L.vsc_guides_hdr(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(edits) if n_e else None, n_e, ch, None, None,
                                            _lib.ptr(pairs), 0 if pairs is None else len(pairs), C.byref(count), None, C.byref(st)), ctx._h)
                wall = (time.perf_counter() - t0) * 1e3
                t = ctx.timing()
                return wall, t["score_ms"], t["scan_ms"]

            runs = timed(once)
            kernel = sorted(r[1] for r in runs)
            out = {"candidates": n, "edits": n_e, "cds": bool(with_cds), "stats": st.as_dict(), "rows_kernel_ms": kernel,
                   "wall_ms": sorted(r[0] for r in runs), "rows_floor_hbm_ms": hbm_rows_ms, "rows_kernel_over_hbm_floor": kernel[0] / hbm_rows_ms,
                   "rows_kernel_over_enumerate_kernels": kernel[0] / enum_ms, "rows_kernel_over_prime_rows_kernel": kernel[0] / prime_ms[key][0]}
            if n_e:
                out.update(pairs_passes_ms=sorted(r[2] for r in runs), pairs_written=bool(write_pairs))
            report(name, out)

    for key, edits in sets:
        for with_cds in (False, True):
            hdr_step("rows_%s%s" % (key, "_cds" if with_cds else ""), key, edits, with_cds, False)
    hdr_step("pairs_snv_cds", "snv", random_edits, True, True)

    with step_limit("filter", args.step_seconds):
        def filter_once():
            out = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_filter_hdr(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(random_edits), len(random_edits), cds._h, None, 0,
                                               C.byref(out)), ctx._h)
            wall = (time.perf_counter() - t0) * 1e3
            kept = int(L.vsc_guides_count(out))
            L.vsc_guides_free(out)
            t = ctx.timing()
            return wall, t["score_ms"], kept, t["genome_bytes"]

        runs = timed(filter_once)
        with_usable = res["rows_snv_cds"]["stats"]["with_usable"]
        assert runs[0][2] == with_usable, (runs[0][2], with_usable)
        report("filter", {"candidates": n, "edits": len(random_edits), "survivors": runs[0][2], "kernels_ms": sorted(r[1] for r in runs),
                          "wall_ms": sorted(r[0] for r in runs), "bytes": runs[0][3],
                          "floor_ms_at_float4_copy_kernel": runs[0][3] / (FLOAT4_COPY_TBS * 1e12) * 1e3})
    L.vsc_guides_free(h)
    genome.close()
    cds.close()
    ctx.close()


if __name__ == "__main__":
    main()

"""Known variation under candidate guides (vsc_guides_variation, vsc_guides_filter_variation) on the synthetic hg38-sized genome
of varscot_amd.synth, one GPU, all NGG candidates, beside the enumeration that produces the candidates and edit_rows_kernel with
the same number of point targets, in one run and one process.

    python tools/variation_bench.py                      JSON to profiles/variation.json (and stdout)
    python tools/variation_bench.py --calls 1 --warmup 1 (what a kernel trace needs: run it under rocprofv3 --kernel-trace --stats)

Steps (each under its own time limit, --step-seconds: W warm-up calls, then K timed calls, fastest .. slowest)
  enumerate        vsc_guides_enumerate alone: NGG, both strands, no filter, no regions; kernels' time = vsc_timing.scan_ms
  edit_1e6 ..      vsc_guides_edit, window (3, 5), base C, with 10^6, 10^7, 10^8 random point targets: edit_rows_kernel =
                   vsc_timing.score_ms - the yardstick, the parent's code
  rows_1e6 ..      vsc_guides_variation, the SpCas9 shape, with as many synthetic variants (nine SNVs to one deletion of 2 .. 50 bases
                   at random positions, a weight each), pairs counted only: var_rows_kernel = vsc_timing.score_ms, the pairs' count pass +
                   scan + write pass (for the coverage) = vsc_timing.scan_ms; the call's wall time holds the upload and the build of the
                   records and the block table
  full_1e8         the 10^8 rows with the lookup's block at 2^32 positions: the plain lower bound over all of `reach`
                   (vsc_debug_variation_block_bits), beside the default block of 256
  pairs_1e6        the 10^6 call with the pairs written and copied to the host
  filter           vsc_guides_filter_variation with the 10^7 variants: nothing in seed or PAM; both passes and the scan
  host             the host route over the first --host-candidates candidates: copy the loci out, numpy.searchsorted on the starts
                   plus the prefix maximum of the ends; scaled to all candidates beside it
Reported beside each kernel time, the floor DERIVED from the shapes: 32 bytes per candidate (16 of locus read, 16 of
row written) plus the block table once, at the 6.3 TB/s a float4 copy kernel reaches."""
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
from efficiency_bench import FLOAT4_COPY_TBS, enumerate_once  # noqa: E402
from microhomology_bench import step_limit  # noqa: E402

BLOCK_BITS = 8  # the library's default block: 256 global positions per table entry


def synthetic_variants(table, span, count, rng):
    """VARIANT_DTYPE of `count` random variants in ascending (contig, pos): nine SNVs to one deletion of 2 .. 50 bases, weights of
    allele frequencies 10^-4 .. 10^-1; what reaches beyond its contig is left out."""
    g = np.sort(rng.integers(0, span, size=count, dtype=np.int64))
    off = np.asarray(table["offset"], dtype=np.int64)
    c = np.searchsorted(off, g, side="right") - 1
    pos = g - off[c]
    deletion = rng.integers(0, 10, size=count) == 0
    spans = np.where(deletion, rng.integers(2, 51, size=count), 1)
    ok = pos + spans <= np.asarray(table["length"], dtype=np.int64)[c]
    alt = np.where(deletion, va.VARIANT_OTHER, rng.integers(0, 4, size=count))
    out = np.zeros(int(ok.sum()), dtype=va.VARIANT_DTYPE)
    out["contig"], out["pos"] = c[ok], pos[ok]
    out["span_alt"] = (spans | alt << 16)[ok]
    out["weight"] = va.variant_weight(10.0 ** rng.uniform(-4, -1, size=count))[ok]
    return out, g[ok], (g + spans)[ok]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--counts", default="1000000,10000000,100000000", help="the numbers of variants (and of point targets)")
    ap.add_argument("--host-candidates", type=int, default=1 << 24)
    ap.add_argument("--step-seconds", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variation.json"))
    args = ap.parse_args()
    sizes = [int(x) for x in args.counts.split(",")]
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    print(json.dumps({"planes_words": int(len(hi))}), flush=True)
    with step_limit("load", args.step_seconds):
        ctx = va.Context(0)
        genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    L = va.lib()
    params = _enum_params("GG", "both", (0, 0), 0, 0)
    table_bytes = 4.0 * (span >> BLOCK_BITS)
    res = {"genome_bases": args.bases, "calls": args.calls, "warmup": args.warmup, "float4_copy_tbs": FLOAT4_COPY_TBS, "block_bits": BLOCK_BITS,
           "block_table_bytes": table_bytes, "plane_bytes": 12.0 * n_words}

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
    floor_ms = (32.0 * n + table_bytes) / (FLOAT4_COPY_TBS * 1e12) * 1e3
    edit_floor_ms = 24.0 * n / (FLOAT4_COPY_TBS * 1e12) * 1e3
    count = C.c_uint64()
    edit_shape, edit_st = va.EDITORS["CBE"]._struct(), _lib.EditStats()
    shape, st = va.VARIATION_SHAPES["SpCas9"]._struct(), _lib.VariationStats()
    rng = np.random.default_rng(32)
    kept = {}

    def rows_once(var, pairs=None):
        t0 = time.perf_counter()
        _lib.check(L.vsc_guides_variation(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(var), len(var), None, _lib.ptr(pairs),
                                          0 if pairs is None else len(pairs), C.byref(count), None, C.byref(st)), ctx._h)
        wall = (time.perf_counter() - t0) * 1e3
        t = ctx.timing()
        return wall, t["score_ms"], t["scan_ms"]

    for size in sizes:
        tag = "1e%d" % round(np.log10(size))
        with step_limit("edit_" + tag, args.step_seconds):
            targets = targets_of_global(table, np.unique(rng.integers(0, span, size=size, dtype=np.int64)))

            def edit_once():
                t0 = time.perf_counter()
                _lib.check(L.vsc_guides_edit(ctx._h, genome._h, h, C.byref(edit_shape), _lib.ptr(targets), len(targets), None, None, 0, C.byref(count),
                                             None, C.byref(edit_st)), ctx._h)
                return (time.perf_counter() - t0) * 1e3, ctx.timing()["score_ms"]

            runs = timed(edit_once)
            report("edit_" + tag, {"candidates": n, "targets": len(targets), "stats": edit_st.as_dict(), "rows_kernel_ms": sorted(r[1] for r in runs),
                                   "wall_ms": sorted(r[0] for r in runs), "rows_floor_hbm_ms": edit_floor_ms})
            del targets
        with step_limit("rows_" + tag, args.step_seconds):
            var, starts, ends = synthetic_variants(table, span, size, rng)
            kept[tag] = (var, starts, ends)
            runs = timed(lambda: rows_once(var))
            kernel = sorted(r[1] for r in runs)
            report("rows_" + tag, {"candidates": n, "variants": len(var), "stats": st.as_dict(), "rows_kernel_ms": kernel,
                                   "pairs_passes_ms": sorted(r[2] for r in runs), "wall_ms": sorted(r[0] for r in runs), "rows_floor_hbm_ms": floor_ms,
                                   "rows_kernel_over_edit_rows_kernel": kernel[0] / res["edit_" + tag]["rows_kernel_ms"][0],
                                   "rows_kernel_over_enumerate_kernels": kernel[0] / res["enumerate"]["kernels_ms"][0]})
    largest = "1e%d" % round(np.log10(sizes[-1]))
    with step_limit("full_" + largest, args.step_seconds):
        var = kept[largest][0]
        _lib.check(L.vsc_debug_variation_block_bits(ctx._h, 32), ctx._h)
        try:
            runs = timed(lambda: rows_once(var))
        finally:
            _lib.check(L.vsc_debug_variation_block_bits(ctx._h, 0), ctx._h)
        kernel = sorted(r[1] for r in runs)
        report("full_" + largest, {"variants": len(var), "block_bits": 32, "stats": st.as_dict(), "rows_kernel_ms": kernel,
                                   "wall_ms": sorted(r[0] for r in runs),
                                   "block_table_over_full_lower_bound": res["rows_" + largest]["rows_kernel_ms"][0] / kernel[0]})
    smallest = "1e%d" % round(np.log10(sizes[0]))
    with step_limit("pairs_" + smallest, args.step_seconds):
        var = kept[smallest][0]
        rows_once(var)
        pairs = np.empty(int(count.value), dtype=va.VARIATION_PAIR_DTYPE)
        runs = timed(lambda: rows_once(var, pairs))
        report("pairs_" + smallest, {"variants": len(var), "pairs": len(pairs), "pairs_passes_ms": sorted(r[2] for r in runs),
                                     "wall_ms": sorted(r[0] for r in runs),
                                     "pairs_floor_hbm_ms": (32.0 * n + 16.0 * len(pairs)) / (FLOAT4_COPY_TBS * 1e12) * 1e3})
        del pairs
    middle = "1e%d" % round(np.log10(sizes[len(sizes) // 2]))
    with step_limit("filter", args.step_seconds):
        var = kept[middle][0]
        f = _lib.VariationFilterStruct(0xFFFFFFFF, 255 | 255 << 8, 0, 0)  # nothing in seed or PAM

        def filter_once():
            out = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_filter_variation(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(var), len(var), C.byref(f), C.byref(out)), ctx._h)
            wall = (time.perf_counter() - t0) * 1e3
            survivors = int(L.vsc_guides_count(out))
            L.vsc_guides_free(out)
            t = ctx.timing()
            return wall, t["score_ms"], survivors, t["genome_bytes"]

        runs = timed(filter_once)
        report("filter", {"candidates": n, "variants": len(var), "survivors": runs[0][2], "kernels_ms": sorted(r[1] for r in runs),
                          "wall_ms": sorted(r[0] for r in runs), "bytes": runs[0][3],
                          "floor_ms_at_float4_copy_kernel": runs[0][3] / (FLOAT4_COPY_TBS * 1e12) * 1e3})
    with step_limit("host", args.step_seconds):
        m = min(n, args.host_candidates)
        off = np.asarray(table["offset"], dtype=np.int64)
        _, starts, ends = kept[smallest]
        reach = np.maximum.accumulate(ends)

        def host_once():
            t0 = time.perf_counter()
            pc, pl = C.c_void_p(), C.c_void_p()
            _lib.check(L.vsc_guides_data(h, C.byref(pc), C.byref(pl)), ctx._h)  # (the first call copies all loci out)
            t1 = time.perf_counter()
            loci = np.frombuffer((C.c_char * (m * 16)).from_address(pl.value), dtype=va.LOCUS_DTYPE)
            g0 = off[loci["contig"]] + loci["pos"].astype(np.int64)
            first = np.searchsorted(reach, g0, side="right")  # the first variant that reaches behind g0
            behind = np.searchsorted(starts, g0 + 23)          # the first variant that starts behind the site
            return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, int((behind > first).sum())

        runs = [host_once() for _ in range(1 + args.calls)]
        join = sorted(r[0] - r[1] for r in runs[1:])
        report("host", {"candidates_joined": m, "variants": len(starts), "copy_out_all_loci_ms": runs[0][1], "join_ms": join,
                        "join_ms_scaled_to_all_candidates": join[0] * n / m, "sites_with_a_candidate_variant": runs[0][2],
                        "note": "the range of candidate variants only: no overlap test, no zones, no alleles, no weights - less than the device computes"})
    L.vsc_guides_free(h)
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()

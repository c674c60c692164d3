"""Coding consequences of base edits (vsc_guides_effects, vsc_guides_filter_effects) on the synthetic hg38-sized genome of
varscot_amd.synth, one GPU, beside edit_rows_kernel without targets over the same candidates, in one run and one process.

    python tools/effects_bench.py                      JSON to profiles/effects.json (and stdout)
    python tools/effects_bench.py --calls 1 --warmup 1 (what a kernel trace needs: run it under rocprofv3 --kernel-trace --stats)

The candidates are edit_bench.py's: NGG, both strands, no filter.  The CDS: every exon-like interval of synth.synthetic_regions
(250 000 intervals, 3 % of the genome; those that overlap an earlier one are dropped) as a one-segment transcript, strands
alternating, phase 0.

Steps (each under its own time limit, --step-seconds: W warm-up calls, then K timed calls, fastest .. slowest)
  enumerate     vsc_guides_enumerate alone - where the candidates come from
  edit_rows     vsc_guides_edit, window (3, 5), base C, no targets: edit_rows_kernel = vsc_timing.score_ms - the yardstick
  rows_exons    vsc_guides_effects, the same window, C -> T, the exon CDS, effects counted only: effects_rows_kernel =
                vsc_timing.score_ms; vsc_timing.scan_ms = the records' count pass + scan and - because the stats are asked for
                and stop_gained effects exist - the write pass that takes the coverage, without records
  rows_one      the same against a CDS of ONE segment: the search is one step, every candidate's walk ends at once - what
                the kernel costs without the segment search
  rows_2500     the same against every hundredth exon: 7 fewer steps of the lower bound than rows_exons
  records       rows_exons with the effects written, the coverage taken and both copied to the host: count pass + scan +
                write pass = vsc_timing.scan_ms
  filter        vsc_guides_filter_effects, require stop_gained: both passes and the scan = vsc_timing.score_ms
Reported beside each kernel time, the floors DERIVED from the shapes: 24 bytes per candidate (16 of locus read, 8
of row written) for the rows kernel, 8 bytes per candidate per records pass that ran (records_launches counts them with the scan:
count pass, scan, and the write pass when records are written or stop_gained effects exist) + 16 per effect written, at the
6.3 TB/s a float4 copy kernel reaches."""
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
from efficiency_bench import FLOAT4_COPY_TBS, enumerate_once  # noqa: E402
from microhomology_bench import step_limit  # noqa: E402


class Table:
    """What va.Cds needs of a genome: its contig table."""

    def __init__(self, contigs):
        self.contigs = contigs


def exon_segments(table, intervals, fraction):
    """CDS_SEGMENT_DTYPE: the exon-like intervals in (contig, start) order without those that overlap an earlier one, each a
    transcript of its own."""
    iv = synth.synthetic_regions(table, intervals, fraction)
    order = np.lexsort((iv["start"], iv["contig"]))
    iv = iv[order]
    keep = np.ones(len(iv), dtype=bool)
    end, contig = 0, -1
    for i in range(len(iv)):
        c, s, e = int(iv["contig"][i]), int(iv["start"][i]), int(iv["end"][i])
        if c != contig:
            contig, end = c, 0
        if s < end or s >= e:
            keep[i] = False
        else:
            end = e
    iv = iv[keep]
    sg = np.zeros(len(iv), dtype=_lib.CDS_SEGMENT_DTYPE)
    sg["contig"], sg["start"], sg["end"] = iv["contig"], iv["start"], iv["end"]
    sg["transcript"] = np.arange(len(iv), dtype=np.uint32)
    sg["strand"] = np.arange(len(iv), dtype=np.uint32) & 1
    return sg


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--intervals", type=int, default=250_000)
    ap.add_argument("--fraction", type=float, default=0.03)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "effects.json"))
    args = ap.parse_args()
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    print(json.dumps({"planes_words": int(len(hi))}), flush=True)
    exons = exon_segments(table, args.intervals, args.fraction)
    sets = {"exons": exons, "one": exons[len(exons) // 2:len(exons) // 2 + 1].copy(), "2500": exons[::100].copy()}
    for sg in sets.values():
        sg["transcript"] = np.arange(len(sg), dtype=np.uint32)
    cds = {k: va.Cds(Table(table), sg, n_tx=len(sg), sort=False) for k, sg in sets.items()}
    print(json.dumps({"segments": {k: len(sg) for k, sg in sets.items()}, "coding_bases": cds["exons"].info()["coding_bases"]}), flush=True)
    with step_limit("load", args.step_seconds):
        ctx = va.Context(0)
        genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    L = va.lib()
    params = _enum_params("GG", "both", (0, 0), 0, 0)
    res = {"genome_bases": args.bases, "calls": args.calls, "warmup": args.warmup, "float4_copy_tbs": FLOAT4_COPY_TBS,
           "segments": {k: len(sg) for k, sg in sets.items()}}

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
    rows = np.empty((n, 2), dtype=np.uint32)
    shape = va.EDITORS["CBE"]._struct()
    to = "ACGT".index(va.EDITOR_TO["CBE"])
    floor_rows_ms = 24.0 * n / (FLOAT4_COPY_TBS * 1e12) * 1e3
    count = C.c_uint64()

    with step_limit("edit_rows", args.step_seconds):
        est = _lib.EditStats()

        def edit_once():
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_edit(ctx._h, genome._h, h, C.byref(shape), None, 0, _lib.ptr(rows), None, 0, C.byref(count), None, C.byref(est)),
                       ctx._h)
            return (time.perf_counter() - t0) * 1e3, ctx.timing()["score_ms"]

        runs = timed(edit_once)
        report("edit_rows", {"candidates": n, "rows_kernel_ms": sorted(r[1] for r in runs), "wall_ms": sorted(r[0] for r in runs),
                             "rows_floor_hbm_ms": floor_rows_ms, "stats": est.as_dict()})
    edit_ms = res["edit_rows"]["rows_kernel_ms"]
    st = _lib.EffectsStats()

    def effects_step(name, which, write):
        with step_limit(name, args.step_seconds):
            c = cds[which]
            effects = cov = None
            if write:
                _lib.check(L.vsc_guides_effects(ctx._h, genome._h, h, C.byref(shape), to, c._h, None, None, None, 0, C.byref(count), None, None),
                           ctx._h)
                effects = np.empty(int(count.value), dtype=va.EFFECT_DTYPE)
                cov = np.empty((c.n_tx, 2), dtype=np.uint32)

            def once():
                t0 = time.perf_counter()
                _lib.check(L.vsc_guides_effects(ctx._h, genome._h, h, C.byref(shape), to, c._h, None, _lib.ptr(rows), _lib.ptr(effects),
                                                0 if effects is None else len(effects), C.byref(count), _lib.ptr(cov), C.byref(st)), ctx._h)
                wall = (time.perf_counter() - t0) * 1e3
                t = ctx.timing()
                return wall, t["score_ms"], t["scan_ms"]

            runs = timed(once)
            kernel = sorted(r[1] for r in runs)
            # the write pass runs for the records, and for the coverage behind the stats whenever a stop_gained effect exists
            wrote = write or (st.effects > 0 and st.by_class[2] > 0)
            passes = 3 if wrote else 2  # count pass, scan[, write pass]
            pass_bytes = 8.0 * n * (2 if wrote else 1) + (16.0 * st.effects if write else 0.0)
            report(name, {"candidates": n, "segments": len(sets[which]), "stats": st.as_dict(), "rows_kernel_ms": kernel,
                          "rows_kernel_median_ms": kernel[len(kernel) // 2], "wall_ms": sorted(r[0] for r in runs),
                          "rows_floor_hbm_ms": floor_rows_ms, "rows_kernel_over_floor": kernel[0] / floor_rows_ms,
                          "rows_kernel_over_edit_rows_kernel": [k / e for k, e in zip(kernel, edit_ms)],
                          "records_passes_ms": sorted(r[2] for r in runs), "records_written": bool(write), "records_launches": passes,
                          "records_floor_hbm_ms": pass_bytes / (FLOAT4_COPY_TBS * 1e12) * 1e3})

    effects_step("rows_exons", "exons", False)
    effects_step("rows_one", "one", False)
    effects_step("rows_2500", "2500", False)
    effects_step("records", "exons", True)

    with step_limit("filter", args.step_seconds):
        def filter_once():
            out = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_filter_effects(ctx._h, genome._h, h, C.byref(shape), to, cds["exons"]._h, None,
                                                   va.effect_class_mask("stop_gained"), 0, C.byref(out)), ctx._h)
            wall = (time.perf_counter() - t0) * 1e3
            kept = int(L.vsc_guides_count(out))
            L.vsc_guides_free(out)
            t = ctx.timing()
            return wall, t["score_ms"], kept, t["genome_bytes"]

        runs = timed(filter_once)
        report("filter", {"candidates": n, "survivors": runs[0][2], "kernels_ms": sorted(r[1] for r in runs),
                          "wall_ms": sorted(r[0] for r in runs), "bytes": runs[0][3],
                          "floor_ms_at_float4_copy_kernel": runs[0][3] / (FLOAT4_COPY_TBS * 1e12) * 1e3})
    L.vsc_guides_free(h)
    for c in cds.values():
        c.close()
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()

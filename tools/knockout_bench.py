"""Knock-out design (vsc_guides_knockout, vsc_guides_filter_knockout) on the synthetic hg38-sized genome of varscot_amd.synth,
one GPU, beside effects_rows_kernel and vsc_guides_enumerate over the same candidates, in one run and one process.

    python tools/knockout_bench.py                      JSON to profiles/knockout.json (and stdout)
    python tools/knockout_bench.py --calls 1 --warmup 1 (what a kernel trace needs: run it under rocprofv3 --kernel-trace --stats)

The candidates are effects_bench.py's: NGG, both strands, no filter.  The CDS: the exon-like intervals of
synth.synthetic_regions (250 000 intervals, 3 % of the genome; those that overlap an earlier one are dropped), once as
one-segment transcripts (no junction: nothing is NMD) and once grouped 8 per transcript in genome order on one contig, strands
alternating per transcript, first phase 0 and the later phases continuing the frame, so that junctions exist.

Steps (each under its own time limit, --step-seconds: W warm-up calls, then K timed calls, fastest .. slowest)
  enumerate      vsc_guides_enumerate alone - where the candidates come from, a yardstick
  effects_rows   vsc_guides_effects, window (3, 5), C -> T, the one-segment CDS: effects_rows_kernel = vsc_timing.score_ms - a yardstick
  rows_one       vsc_guides_knockout, SpCas9 shape, the one-segment CDS: knockout_rows_kernel = vsc_timing.score_ms
  rows_8         the same against the CDS grouped 8 per transcript, with the coverage
  in_place_8     rows_8 with the queue taken out (vsc_debug_knockout_in_place): every coding lane walks where it lies
  filter         vsc_guides_filter_knockout on the grouped CDS, 5 % .. 65 % of the protein with NMD in both frames: both passes
                 and the scan = vsc_timing.score_ms
Reported beside each kernel time: the share of the defined candidates that the occupancy bitmap sends past cds_find, the drains
of the queue and their mean fill (lanes busy in a walk, of 64), and the floor DERIVED from the shapes: 32 bytes per
candidate (16 of locus read, 16 of row written) at the 6.3 TB/s a float4 copy kernel reaches."""
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
from effects_bench import Table, exon_segments  # noqa: E402
from efficiency_bench import FLOAT4_COPY_TBS, enumerate_once  # noqa: E402
from microhomology_bench import step_limit  # noqa: E402


def grouped(exons, per_transcript):
    """The exon segments with every `per_transcript` consecutive ones of a contig as one transcript: one strand per transcript
    (alternating), first phase 0, the later phases continuing the reading frame in transcript order."""
    sg = exons.copy()
    n = len(sg)
    tx = np.zeros(n, dtype=np.uint32)
    at, t = 0, 0
    while at < n:
        c = sg["contig"][at]
        end = at
        while end < n and end - at < per_transcript and sg["contig"][end] == c:
            end += 1
        tx[at:end] = t
        strand = t & 1
        order = range(end - 1, at - 1, -1) if strand else range(at, end)
        ci = 0
        for i in order:
            sg["strand"][i] = strand
            sg["phase"][i] = (3 - ci % 3) % 3
            ci += int(sg["end"][i]) - int(sg["start"][i])
        at, t = end, t + 1
    sg["transcript"] = tx
    return sg, t


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--intervals", type=int, default=250_000)
    ap.add_argument("--fraction", type=float, default=0.03)
    ap.add_argument("--per-transcript", type=int, default=8)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knockout.json"))
    args = ap.parse_args()
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    print(json.dumps({"planes_words": int(len(hi))}), flush=True)
    exons = exon_segments(table, args.intervals, args.fraction)
    exons["transcript"] = np.arange(len(exons), dtype=np.uint32)
    eight, n_eight = grouped(exons, args.per_transcript)
    cds = {"one": va.Cds(Table(table), exons, n_tx=len(exons), sort=False), "8": va.Cds(Table(table), eight, n_tx=n_eight, sort=False)}
    print(json.dumps({"segments": len(exons), "transcripts": {"one": len(exons), "8": n_eight},
                      "coding_bases": cds["one"].info()["coding_bases"]}), flush=True)
    with step_limit("load", args.step_seconds):
        ctx = va.Context(0)
        genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    L = va.lib()
    params = _enum_params("GG", "both", (0, 0), 0, 0)
    res = {"genome_bases": args.bases, "calls": args.calls, "warmup": args.warmup, "float4_copy_tbs": FLOAT4_COPY_TBS,
           "segments": len(exons), "transcripts": {"one": len(exons), "8": n_eight}, "bitmap_block_positions": 256}

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
    floor_ms = 32.0 * n / (FLOAT4_COPY_TBS * 1e12) * 1e3
    count = C.c_uint64()

    with step_limit("effects_rows", args.step_seconds):
        rows2 = np.empty((n, 2), dtype=np.uint32)
        eshape = va.EDITORS["CBE"]._struct()
        to = "ACGT".index(va.EDITOR_TO["CBE"])
        est = _lib.EffectsStats()

        def effects_once():
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_effects(ctx._h, genome._h, h, C.byref(eshape), to, cds["one"]._h, None, _lib.ptr(rows2), None, 0, C.byref(count),
                                            None, C.byref(est)), ctx._h)
            return (time.perf_counter() - t0) * 1e3, ctx.timing()["score_ms"]

        runs = timed(effects_once)
        report("effects_rows", {"candidates": n, "rows_kernel_ms": sorted(r[1] for r in runs), "wall_ms": sorted(r[0] for r in runs)})
        del rows2
    effects_ms = res["effects_rows"]["rows_kernel_ms"]
    rows = np.empty((n, 4), dtype=np.uint32)
    shape = va.KNOCKOUT_SHAPES["SpCas9"]._struct()
    st = _lib.KnockoutStats()

    def knockout_step(name, which, coverage, in_place=False):
        with step_limit(name, args.step_seconds):
            c = cds[which]
            cov = np.empty((c.n_tx, 2), dtype=np.uint32) if coverage else None

            def once():
                t0 = time.perf_counter()
                _lib.check(L.vsc_guides_knockout(ctx._h, genome._h, h, C.byref(shape), c._h, None, _lib.ptr(rows), _lib.ptr(cov), C.byref(st)), ctx._h)
                return (time.perf_counter() - t0) * 1e3, ctx.timing()["score_ms"]

            _lib.check(L.vsc_debug_knockout_in_place(ctx._h, 1 if in_place else 0), ctx._h)
            try:
                runs = timed(once)
            finally:
                L.vsc_debug_knockout_in_place(ctx._h, 0)
            kernel = sorted(r[1] for r in runs)
            s = st.as_dict()
            report(name, {"candidates": n, "transcripts": c.n_tx, "in_place": in_place, "stats": s, "rows_kernel_ms": kernel,
                          "rows_kernel_median_ms": kernel[len(kernel) // 2], "wall_ms": sorted(r[0] for r in runs),
                          "past_find_share": s["past_find"] / max(s["defined"], 1), "coding_share": s["coding"] / max(s["defined"], 1),
                          "drains": s["drains"], "mean_fill_of_64": s["drained"] / max(s["drains"], 1),
                          "rows_floor_hbm_ms": floor_ms, "rows_kernel_over_floor": kernel[0] / floor_ms,
                          "rows_kernel_over_effects_rows_kernel": [k / e for k, e in zip(kernel, effects_ms)],
                          "rows_kernel_over_enumerate": [k / e for k, e in zip(kernel, res["enumerate"]["kernels_ms"])]})

    knockout_step("rows_one", "one", False)
    knockout_step("rows_8", "8", True)
    knockout_step("in_place_8", "8", True, in_place=True)

    with step_limit("filter", args.step_seconds):
        lim = _lib.KnockoutLimits(va.knockout_cut_frac(0.05), va.knockout_cut_frac(0.65, upper=True), 0, va.knockout_flag_mask("nmd1+nmd2"), 0,
                                  (C.c_uint32 * 3)(0, 0, 0))

        def filter_once():
            out = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_filter_knockout(ctx._h, genome._h, h, C.byref(shape), cds["8"]._h, None, C.byref(lim), C.byref(out)), ctx._h)
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

"""Bulges under a pattern (vsc_search_pattern_bulges) on the synthetic hg38-sized genome of varscot_amd.synth, one GPU.

    python tools/pattern_bulge_bench.py                 all cases, JSON to profiles/pattern_bulges.json (and stdout)
    python tools/pattern_bulge_bench.py --calls 1 --warmup 0 --out /tmp/x.json     (what a kernel trace needs: run it under
                                                         rocprofv3 --kernel-trace --stats; --stats-csv FILE then adds the trace)

16 synthetic guides at 4 mismatches, records and rows both asked for.  The cases:
    plain23-u1,1 / plain23-u2,2   N x 21 + GR with the 23 letters of every guide spelled, protospacer (0, 20): the definition of
                                  vsc_search_bulges, which runs beside it on the same guides in the same process - the yardstick.
                                  The record counts and the rows of the two are asserted equal.
    SaCas9-u1,1                   N x 21 + NNGRRT, protospacer (0, 21)
    Cas12a-u1,1                   TTTV + N x 23, protospacer (4, 23)
Every case: W warm-up calls, then K timed calls, fastest .. slowest: host wall time per call and the kernels' own time
(vsc_timing.scan_ms = count pass + offsets + write pass, between HIP events).  The result stays on the device and is freed again.
Reported per case: candidates (vsc_timing.sites), candidate x guide comparisons per second of kernel time, records, and for the
first two the ratio to vsc_search_bulges' kernels.
--stats-csv: a rocprofv3 kernel_stats.csv of a traced run; its rows for the kernels involved are copied into the JSON under
"kernel_trace".
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import varscot_amd as va  # noqa: E402
from varscot_amd import _lib, dist as vdist, synth  # noqa: E402


def cases_of(guides):
    """name -> (pattern, guides, protospacer, dna, rna)"""
    sa, cas12a = va.pattern_strings("SaCas9")[0], va.pattern_strings("Cas12a")[0]
    return {
        "plain23-u1,1": ("N" * 21 + "GR", list(guides), (0, 20), 1, 1),
        "plain23-u2,2": ("N" * 21 + "GR", list(guides), (0, 20), 2, 2),
        "SaCas9-u1,1": (sa, [g[:21] + "N" * 6 for g in guides], va.pattern_protospacer("SaCas9"), 1, 1),
        "Cas12a-u1,1": (cas12a, ["N" * 4 + g for g in guides], va.pattern_protospacer("Cas12a"), 1, 1),
    }


def pattern_bulge_call(ctx, genome, pattern, guides, m, proto, dna, rna):
    """(wall ms, kernels ms, records, timing, rows) of one vsc_search_pattern_bulges with records and rows; the result is freed"""
    L = va.lib()
    pp = _lib.PatternBulgeParams(m, 0, 0, proto[0], proto[1], dna, rna)
    rows = np.zeros((len(guides), _lib.BULGE_CLASSES, 9), dtype=np.uint32)
    h = C.c_void_p()
    text = "".join(guides).encode()
    t0 = time.perf_counter()
    _lib.check(L.vsc_search_pattern_bulges(ctx._h, genome._h, pattern.encode(), text, len(guides), len(pattern), C.byref(pp), C.byref(h),
                                           _lib.ptr(rows)), ctx._h)
    wall = (time.perf_counter() - t0) * 1e3
    n = int(L.vsc_bulge_hits_count(h))
    L.vsc_bulge_hits_free(h)
    t = ctx.timing()
    assert t["hits"] == n == int(rows.sum())
    return wall, t["scan_ms"], n, t, rows


def bulge_call(ctx, genome, codes, m, dna, rna):
    """the same of one vsc_search_bulges"""
    L = va.lib()
    p = genome._params(m, None, _lib.ALGO_SCAN)
    bp = _lib.BulgeParams(dna, rna, 0, 0, 0)
    rows = np.zeros((len(codes), _lib.BULGE_CLASSES, 9), dtype=np.uint32)
    h = C.c_void_p()
    t0 = time.perf_counter()
    _lib.check(L.vsc_search_bulges(ctx._h, genome._h, _lib.ptr(codes), len(codes), C.byref(p), C.byref(bp), C.byref(h), _lib.ptr(rows)),
               ctx._h)
    wall = (time.perf_counter() - t0) * 1e3
    n = int(L.vsc_bulge_hits_count(h))
    L.vsc_bulge_hits_free(h)
    t = ctx.timing()
    assert t["hits"] == n == int(rows.sum())
    return wall, t["scan_ms"], n, t, rows


def kernel_trace(path):
    want = ("pattern_bulge_", "bulge_count_kernel", "bulge_write_kernel", "bulge_chunk_sum_kernel", "enum_scan_kernel")
    with open(path, newline="") as f:
        return [row for row in csv.DictReader(f) if any(w in row.get("Name", "") for w in want)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--guides", type=int, default=16)
    ap.add_argument("--mismatches", type=int, default=4)
    ap.add_argument("--cases", default="plain23-u1,1;plain23-u2,2;SaCas9-u1,1;Cas12a-u1,1", help="names separated by ';'")
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--stats-csv", default=None, help="kernel_stats.csv of a run of this tool under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pattern_bulges.json"))
    args = ap.parse_args()
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    guides = list(synth.synthetic_guides(args.guides)[1])
    codes = va.pack_guides(guides)
    m = args.mismatches
    res = {"genome_bases": args.bases, "guides": args.guides, "mismatches": m, "calls": args.calls, "warmup": args.warmup, "cases": {},
           "search_bulges": {}}
    table_of = cases_of(guides)
    for name in args.cases.split(";"):
        pattern, gs, proto, dna, rna = table_of[name]
        for _ in range(args.warmup):
            pattern_bulge_call(ctx, genome, pattern, gs, m, proto, dna, rna)
        runs = [pattern_bulge_call(ctx, genome, pattern, gs, m, proto, dna, rna) for _ in range(args.calls)]
        assert len({r[2] for r in runs}) == 1 and all(r[4].tobytes() == runs[0][4].tobytes() for r in runs)
        kernel = sorted(r[1] for r in runs)
        t = runs[0][3]
        case = {"pattern": pattern, "protospacer": list(proto), "dna": dna, "rna": rna, "wall_ms": sorted(r[0] for r in runs), "kernels_ms": kernel,
                "records": runs[0][2], "candidates": t["sites"], "comparisons": t["pairs"], "passes": t["passes"],
                "comparisons_per_s_at_fastest": t["pairs"] / (kernel[0] * 1e-3), "candidates_per_s_at_fastest": t["sites"] / (kernel[0] * 1e-3),
                "rows_by_class_and_nm": runs[0][4].sum(0).tolist()}
        if name.startswith("plain23"):  # the yardstick: vsc_search_bulges on the same guides, here and now
            for _ in range(args.warmup):
                bulge_call(ctx, genome, codes, m, dna, rna)
            ref = [bulge_call(ctx, genome, codes, m, dna, rna) for _ in range(args.calls)]
            assert ref[0][2] == runs[0][2], "record counts differ: %d, vsc_search_bulges %d" % (runs[0][2], ref[0][2])
            assert ref[0][4].tobytes() == runs[0][4].tobytes(), "rows differ from vsc_search_bulges'"
            ref_kernel = sorted(r[1] for r in ref)
            res["search_bulges"]["u%d,%d" % (dna, rna)] = {"wall_ms": sorted(r[0] for r in ref), "kernels_ms": ref_kernel, "records": ref[0][2],
                                                            "candidates": ref[0][3]["sites"]}
            case["ratio_to_search_bulges_kernels"] = kernel[0] / ref_kernel[0]
        res["cases"][name] = case
        print(json.dumps({name: case}), flush=True)
    if args.stats_csv:
        res["kernel_trace"] = kernel_trace(args.stats_csv)
    genome.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""The bulge-tolerant search (vsc_search_bulges) on the synthetic hg38-sized genome of varscot_amd.synth, one GPU.

    python tools/bulge_bench.py                         both cases, JSON to profiles/bulges.json (and stdout)
    python tools/bulge_bench.py --calls 1 --warmup 0 --out /tmp/x.json     (what a kernel trace needs: run it under
                                                         rocprofv3 --kernel-trace --stats; --stats-csv FILE then adds the trace)

16 synthetic guides at 4 mismatches, the cases -u 1,1 and -u 2,2 (largest DNA, RNA bulge), records and rows both asked for.
Every case: W warm-up calls, then K timed calls, fastest .. slowest: host wall time per call and the kernels' own time
(vsc_timing.scan_ms = count pass + offsets + write pass).  The result stays on the device and is freed again.
Beside them, in the same process and on the same resident genome: the plain substitution-only search of the same guides with
VSC_ALGO_SCAN (vsc_search; its scan_ms and total_ms), and the ratio of the two kernels' times.  Reported per case: candidates
(vsc_timing.sites: PAM-valid N-free sites of the enabled classes, both strands), candidate x guide comparisons per second of
kernel time, records.
--stats-csv: a rocprofv3 kernel_stats.csv of a traced run; its rows for the bulge kernels and the scan kernel are copied into
the JSON under "kernel_trace".
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


def bulge_call(ctx, genome, codes, m, dna, rna):
    """(wall ms, kernels ms, records, timing) of one vsc_search_bulges with records and rows; the result is freed"""
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


def plain_call(ctx, genome, codes, m):
    t0 = time.perf_counter()
    hits = genome.search(codes, m, algorithm="scan")
    wall = (time.perf_counter() - t0) * 1e3
    n = len(hits)
    hits.close()
    t = ctx.timing()
    return wall, t["scan_ms"], t["total_ms"], n, t["sites"]


def kernel_trace(path):
    want = ("bulge_", "enum_scan_kernel", "scan_kernel")
    with open(path, newline="") as f:
        return [row for row in csv.DictReader(f) if any(w in row.get("Name", "") for w in want)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--guides", type=int, default=16)
    ap.add_argument("--mismatches", type=int, default=4)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--stats-csv", default=None, help="kernel_stats.csv of a run of this tool under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bulges.json"))
    args = ap.parse_args()
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    codes = va.pack_guides(synth.synthetic_guides(args.guides)[1])
    m = args.mismatches
    res = {"genome_bases": args.bases, "guides": args.guides, "mismatches": m, "calls": args.calls, "warmup": args.warmup, "cases": {}}
    for _ in range(args.warmup):
        plain_call(ctx, genome, codes, m)
    plain = [plain_call(ctx, genome, codes, m) for _ in range(args.calls)]
    res["plain_scan"] = {"wall_ms": sorted(r[0] for r in plain), "scan_kernel_ms": sorted(r[1] for r in plain),
                         "total_ms": sorted(r[2] for r in plain), "hits": plain[0][3], "sites": plain[0][4]}
    print(json.dumps({"plain_scan": res["plain_scan"]}), flush=True)
    for dna, rna in ((1, 1), (2, 2)):
        for _ in range(args.warmup):
            bulge_call(ctx, genome, codes, m, dna, rna)
        runs = [bulge_call(ctx, genome, codes, m, dna, rna) for _ in range(args.calls)]
        assert len({r[2] for r in runs}) == 1 and all(r[4].tobytes() == runs[0][4].tobytes() for r in runs)
        kernel = sorted(r[1] for r in runs)
        t = runs[0][3]
        case = {"wall_ms": sorted(r[0] for r in runs), "kernels_ms": kernel, "records": runs[0][2], "candidates": t["sites"],
                "comparisons": t["pairs"], "passes": t["passes"],
                "comparisons_per_s_at_fastest": t["pairs"] / (kernel[0] * 1e-3), "candidates_per_s_at_fastest": t["sites"] / (kernel[0] * 1e-3),
                "kernels_ms_per_guide": kernel[0] / args.guides,
                "ratio_to_plain_scan_kernel": kernel[0] / res["plain_scan"]["scan_kernel_ms"][0],
                "ratio_to_plain_scan_total": kernel[0] / res["plain_scan"]["total_ms"][0],
                "rows_by_class_and_nm": runs[0][4].sum(0).tolist()}
        res["cases"]["u%d,%d" % (dna, rna)] = case
        print(json.dumps({"u%d,%d" % (dna, rna): case}), flush=True)
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

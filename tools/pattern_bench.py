"""The pattern search (vsc_search_pattern) on the synthetic hg38-sized genome of varscot_amd.synth, one GPU.

    python tools/pattern_bench.py                       all cases, JSON to profiles/pattern.json (and stdout)
    python tools/pattern_bench.py --calls 1 --warmup 0 --out /tmp/x.json     (what a kernel trace needs: run it under
                                                         rocprofv3 --kernel-trace --stats; --stats-csv FILE then adds the trace)

16 synthetic guides, records and rows both asked for, the cases
    plain23   pattern N x 21 + GR with the 23-letter guides at m = 4: the hit set of the plain search up to the right-edge rule
    SaCas9    N x 21 + NNGRRT, the guides' first 21 letters + N x 6, m = 4 (L = 27)
    Cas12a    TTTV + N x 23, N x 4 + the guides, m = 4 (L = 27)
    trunc17   N x 17 + NGG, the guides' first 17 letters + N x 3, m = 3 (L = 20)
Every case: W warm-up calls, then K timed calls, fastest .. slowest: host wall time per call and the kernels' own time
(vsc_timing.scan_ms = count pass + offsets + write pass).  The result stays on the device and is freed again.
Beside them, in the same process and on the same resident genome: the plain substitution-only search of the same guides with
VSC_ALGO_SCAN (vsc_search; its scan_ms and total_ms), and the ratio of the two kernels' times.  Reported per case: candidates
(vsc_timing.sites: sites that satisfy the pattern and hold no N, both strands), candidate x guide comparisons per second of
kernel time, records.
--stats-csv: a rocprofv3 kernel_stats.csv of a traced run; its rows for the pattern kernels, the offset kernels and the scan
kernel are copied into the JSON under "kernel_trace".
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
    """name -> (pattern, guides, m)"""
    sa, _ = va.pattern_strings("SaCas9")
    cas12a, _ = va.pattern_strings("Cas12a")
    return {
        "plain23": ("N" * 21 + "GR", list(guides), 4),
        "SaCas9": (sa, [g[:21] + "N" * 6 for g in guides], 4),
        "Cas12a": (cas12a, ["N" * 4 + g for g in guides], 4),
        "trunc17": ("N" * 17 + "NGG", [g[:17] + "NNN" for g in guides], 3),
    }


def pattern_call(ctx, genome, pattern, guides, m):
    """(wall ms, kernels ms, records, timing, rows) of one vsc_search_pattern with records and rows; the result is freed"""
    L = va.lib()
    pp = _lib.PatternParams(m, 0, 0)
    rows = np.zeros((len(guides), 9), dtype=np.uint32)
    h = C.c_void_p()
    text = "".join(guides).encode()
    t0 = time.perf_counter()
    _lib.check(L.vsc_search_pattern(ctx._h, genome._h, pattern.encode(), text, len(guides), len(pattern), C.byref(pp), C.byref(h),
                                    _lib.ptr(rows)), ctx._h)
    wall = (time.perf_counter() - t0) * 1e3
    n = int(L.vsc_pattern_hits_count(h))
    L.vsc_pattern_hits_free(h)
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
    want = ("pattern_", "bulge_chunk_sum_kernel", "enum_scan_kernel", "scan_kernel")
    with open(path, newline="") as f:
        return [row for row in csv.DictReader(f) if any(w in row.get("Name", "") for w in want)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--guides", type=int, default=16)
    ap.add_argument("--cases", default="plain23,SaCas9,Cas12a,trunc17")
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--stats-csv", default=None, help="kernel_stats.csv of a run of this tool under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pattern.json"))
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
    res = {"genome_bases": args.bases, "guides": args.guides, "calls": args.calls, "warmup": args.warmup, "cases": {}}
    for _ in range(args.warmup):
        plain_call(ctx, genome, codes, 4)
    plain = [plain_call(ctx, genome, codes, 4) for _ in range(args.calls)]
    res["plain_scan"] = {"mismatches": 4, "wall_ms": sorted(r[0] for r in plain), "scan_kernel_ms": sorted(r[1] for r in plain),
                         "total_ms": sorted(r[2] for r in plain), "hits": plain[0][3], "sites": plain[0][4]}
    print(json.dumps({"plain_scan": res["plain_scan"]}), flush=True)
    table_of = cases_of(guides)
    for name in args.cases.split(","):
        pattern, gs, m = table_of[name]
        for _ in range(args.warmup):
            pattern_call(ctx, genome, pattern, gs, m)
        runs = [pattern_call(ctx, genome, pattern, gs, m) for _ in range(args.calls)]
        assert len({r[2] for r in runs}) == 1 and all(r[4].tobytes() == runs[0][4].tobytes() for r in runs)
        kernel = sorted(r[1] for r in runs)
        t = runs[0][3]
        case = {"pattern": pattern, "length": len(pattern), "mismatches": m, "wall_ms": sorted(r[0] for r in runs), "kernels_ms": kernel,
                "records": runs[0][2], "candidates": t["sites"], "comparisons": t["pairs"], "passes": t["passes"],
                "comparisons_per_s_at_fastest": t["pairs"] / (kernel[0] * 1e-3), "candidates_per_s_at_fastest": t["sites"] / (kernel[0] * 1e-3),
                "ratio_to_plain_scan_kernel": kernel[0] / res["plain_scan"]["scan_kernel_ms"][0],
                "ratio_to_plain_scan_total": kernel[0] / res["plain_scan"]["total_ms"][0],
                "rows_by_nm": runs[0][4].sum(0).tolist()}
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

"""Per-guide summary (vsc_search_summary) against the record path, on bench.py's workloads, one GPU.

    python tools/summary_bench.py --workload c3 --steps 3 --warmup 1      one JSON line per workload on stdout
    python tools/summary_bench.py --workload c3 --steps 1 --warmup 1 --summary-only     (what a kernel trace needs)

The inputs are made as bench.py makes them (varscot_amd.synth: same contig table, planes, guides and seeds; the seed index
built before the timed steps), and a step is timed the same way: W untimed steps, then K steps, host wall time per step.
  summary  Genome.summarize(guides, 8): search, then summary_kernel over the records where they lie
  records  c3: Genome.search(guides, 8) (search + bin sort + finalize into 16-byte records, freed again);
           c5: Genome.search_streamed in batches of 10 000 with a callback that does nothing (bench.py's c5 route without
           its per-hit feature rows: the cheapest way to the records)
vsc_timing of the last step of each is reported beside the wall times (summary: sort_ms = 0, finalize_ms = summary_kernel).
--regions N,FRACTION adds the region-aware summary (vsc_search_summary_regions) over a synthetic annotation of N random
intervals that together cover FRACTION of the genome (varscot_amd.synth.synthetic_regions; 250000,0.03 is exon-like): its
steps (fastest .. slowest beside the plain summary's), their ratio to the plain step of the same process, the share of the
hits in the regions and the class table's block size and class counts (vsc_regions_info).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import varscot_amd as va  # noqa: E402
from varscot_amd import dist as vdist, synth  # noqa: E402

WORKLOADS = {"c3": (10_000, 3_000_000_000, 8), "c5": (100_000, 3_000_000_000, 8)}  # bench.py's WORKLOADS
SPLIT = ("scan_ms", "prep_ms", "sort_ms", "finalize_ms", "total_ms", "hits", "passes", "read_passes", "sites", "algorithm")


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    return (time.perf_counter() - t0) * 1e3 / steps, out


def timed_each(fn, steps, warmup):
    """as timed(), every step on its own: ({mean, min, max} in ms, last result)"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"mean": sum(ms) / len(ms), "min": min(ms), "max": max(ms)}, out


def parse_regions(text):
    n, fraction = text.split(",")
    return int(n), float(fraction)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS) + ["both"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=10_000, help="c5 record path: reads per streamed batch (bench.py --batch)")
    ap.add_argument("--summary-only", action="store_true", help="time the summary path only")
    ap.add_argument("--regions", type=parse_regions, metavar="N,FRACTION",
                    help="also time the region-aware summary over N random intervals covering FRACTION of the genome")
    ap.add_argument("--rule", default="overlap", choices=["overlap", "inside"], help="--regions: the membership rule")
    args = ap.parse_args()
    names = ["c3", "c5"] if args.workload == "both" else [args.workload]
    total_bases = WORKLOADS[names[0]][1]
    table, _ = synth.contig_table(total_bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(total_bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    genome.build_index()
    regions = None
    if args.regions:
        regions = va.Regions(va.PackedGenome(None, None, None, table), synth.synthetic_regions(table, *args.regions), rule=args.rule)
    for name in names:
        n_guides, _, max_mm = WORKLOADS[name]
        _, seqs = synth.synthetic_guides(n_guides)
        codes = va.pack_guides(seqs)

        ms_sum, rows = timed(lambda: genome.summarize(codes, max_mm, algorithm="seed"), args.steps, args.warmup)
        t_sum = ctx.timing()
        counted = int(rows["nm"].sum())
        res = {"workload": name, "guides": n_guides, "max_mismatches": max_mm, "genome_bases": total_bases, "steps": args.steps,
               "warmup": args.warmup, "summary_ms_per_step": ms_sum, "summary_timing": {k: t_sum[k] for k in SPLIT},
               "summary_kernel_ms": t_sum["finalize_ms"], "summary_hits": counted,
               "summary_record_bytes": 8 * counted, "mit_specificity_median": float(np.median(
                   [va.mit_specificity(int(x)) for x in rows["mit_sum"][:2000]]))}
        if regions is not None:
            plain_ms, _ = timed_each(lambda: genome.summarize(codes, max_mm, algorithm="seed"), args.steps, args.warmup)
            reg_ms, (rows_all, rows_in) = timed_each(lambda: genome.summarize(codes, max_mm, algorithm="seed", regions=regions),
                                                     args.steps, args.warmup)
            t_reg = ctx.timing()
            res["regions"] = {"intervals": args.regions[0], "fraction": args.regions[1], "rule": args.rule, "info": regions.info(),
                              "plain_ms_per_step": plain_ms, "regions_ms_per_step": reg_ms,
                              "regions_vs_plain": reg_ms["mean"] / plain_ms["mean"], "summary_kernel_ms": t_reg["finalize_ms"],
                              "plain_summary_kernel_ms": t_sum["finalize_ms"], "hits_in_regions": int(rows_in["nm"].sum()),
                              "hits": int(rows_all["nm"].sum()), "all_rows_equal_plain": rows_all.tobytes() == rows.tobytes()}
        if not args.summary_only:
            if name == "c5":
                got = [0]

                def records():
                    got[0] = 0

                    def on_batch(h, first, count):
                        got[0] += len(h)
                    genome.search_streamed(codes, max_mm, on_batch, batch=args.batch, algorithm="seed")
                    return got[0]
            else:
                def records():
                    h = genome.search(codes, max_mm, algorithm="seed")
                    n = len(h)
                    h.close()
                    return n
            ms_rec, n_rec = timed(records, args.steps, args.warmup)
            t_rec = ctx.timing()
            res.update({"records_ms_per_step": ms_rec, "records_timing": {k: t_rec[k] for k in SPLIT}, "records_hits": n_rec,
                        "records_route": "vsc_search_stream, batches of %d, no scoring" % args.batch if name == "c5"
                        else "vsc_search (search + bin sort + finalize)",
                        "summary_vs_records": ms_sum / ms_rec, "same_hits": n_rec == counted})
        print(json.dumps(res), flush=True)
    if regions is not None:
        regions.close()
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()

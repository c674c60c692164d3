"""Per-guide selection (vsc_search_select) against the record path, on bench.py's workloads, one GPU.

    python tools/select_bench.py --workload both --steps 3 --warmup 1     one JSON line per workload on stdout
    python tools/select_bench.py --workload c3 --steps 1 --warmup 1 --select-only --top-k 100    (what a kernel trace needs)

The inputs are made as bench.py makes them (varscot_amd.synth: same contig table, planes, guides and seeds; the seed index
built before the timed steps), and a step is timed as tools/summary_bench.py times it: W untimed steps, then K steps, host
wall time per step (mean, and the fastest and slowest step).
  select   Genome.search_select(guides, 8, top_k=K) for every K of --top-k: search, selection kernels over the records
           where they lie, bin sort + finalize of the survivors
  records  c3: Genome.search(guides, 8); c5: Genome.search_streamed in batches of 10 000 with a callback that does nothing
Before each path the context's pooled scratch is given back; the device memory the path then takes (free memory before
minus after its steps, results freed: the pooled buffers) is reported as pooled_bytes - the record path's includes the
sort's slot layout and the result's room, the selection's does not.
--regions N,FRACTION adds, for every K, the selection among the hits in a synthetic annotation (vsc_search_select_regions,
scope keep; N random intervals covering FRACTION of the genome as tools/summary_bench.py makes them) and its ratio to the
plain selection of the same process.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import varscot_amd as va  # noqa: E402
from varscot_amd import dist as vdist, synth  # noqa: E402

WORKLOADS = {"c3": (10_000, 3_000_000_000, 8), "c5": (100_000, 3_000_000_000, 8)}  # bench.py's WORKLOADS
SPLIT = ("scan_ms", "prep_ms", "sort_ms", "finalize_ms", "total_ms", "hits", "passes", "read_passes", "sort_bytes", "sort_levels",
         "algorithm")


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"mean": sum(ms) / len(ms), "min": min(ms), "max": max(ms)}, out


def pooled(ctx, fn, steps, warmup):
    """timed(fn) from an empty pool; also the device bytes the context holds afterwards."""
    ctx.release_scratch()
    free0 = torch.cuda.mem_get_info(0)[0]
    ms, out = timed(fn, steps, warmup)
    return ms, out, free0 - torch.cuda.mem_get_info(0)[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS) + ["both"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--top-k", type=int, nargs="+", default=[20, 100])
    ap.add_argument("--batch", type=int, default=10_000, help="c5 record path: reads per streamed batch (bench.py --batch)")
    ap.add_argument("--select-only", action="store_true", help="time the selection only")
    ap.add_argument("--regions", type=lambda t: (int(t.split(",")[0]), float(t.split(",")[1])), metavar="N,FRACTION",
                    help="also time the selection among the hits in N random intervals covering FRACTION of the genome")
    ap.add_argument("--rule", default="overlap", choices=["overlap", "inside"], help="--regions: the membership rule")
    ap.add_argument("--scope", default="keep", choices=["keep", "drop"], help="--regions: the side the selection is made on")
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
        res = {"workload": name, "guides": n_guides, "max_mismatches": max_mm, "genome_bases": total_bases, "steps": args.steps,
               "warmup": args.warmup, "select": {}}
        for k in args.top_k:
            def step():
                h = genome.search_select(codes, max_mm, top_k=k, algorithm="seed")
                n = len(h)
                h.close()
                return n
            ms, kept, held = pooled(ctx, step, args.steps, args.warmup)
            t = ctx.timing()
            res["select"][str(k)] = {"ms_per_step": ms, "selected": kept, "result_bytes": 16 * kept, "pooled_bytes": held,
                                     "timing": {f: t[f] for f in SPLIT}}
            if regions is not None:
                def step_regions():
                    h = genome.search_select(codes, max_mm, top_k=k, algorithm="seed", regions=regions, region_scope=args.scope)
                    n = len(h)
                    h.close()
                    return n
                ms_r, kept_r, held_r = pooled(ctx, step_regions, args.steps, args.warmup)
                t = ctx.timing()
                res.setdefault("select_regions", {"intervals": args.regions[0], "fraction": args.regions[1], "rule": args.rule,
                                                  "scope": args.scope, "info": regions.info()})[str(k)] = {
                    "ms_per_step": ms_r, "selected": kept_r, "pooled_bytes": held_r, "timing": {f: t[f] for f in SPLIT},
                    "regions_vs_plain": ms_r["mean"] / ms["mean"]}
        if not args.select_only:
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
            ms, n_rec, held = pooled(ctx, records, args.steps, args.warmup)
            t = ctx.timing()
            res["records"] = {"ms_per_step": ms, "hits": n_rec, "pooled_bytes": held, "timing": {f: t[f] for f in SPLIT},
                              "route": "vsc_search_stream, batches of %d, no scoring" % args.batch if name == "c5"
                              else "vsc_search (search + bin sort + finalize)"}
            res["same_hits"] = all(v["timing"]["hits"] == n_rec for v in res["select"].values())
            res["select_vs_records"] = {k: v["ms_per_step"]["mean"] / ms["mean"] for k, v in res["select"].items()}
        print(json.dumps(res), flush=True)
    if regions is not None:
        regions.close()
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()

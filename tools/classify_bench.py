"""Per-guide classifier rows and top-K by votes (vsc_search_summary_classified / vsc_search_select_classified) against the
record route, on bench.py's synthetic genome at 8 mismatches with the shipped forest, one GPU.

    python tools/classify_bench.py --guides 1000 --steps 3 --warmup 1 [--out profiles/classified_c3.json]

The inputs are made as bench.py makes them (varscot_amd.synth: same contig table, planes and seeds, the first --guides of its
guides; the seed index built before the timed steps).  Three routes, timed in interleaved rounds of one process (W untimed
rounds, then K rounds; host wall time per step, every step ends in a device synchronise):
  summary  Genome.summarize_classified: search, classify in place, the two summary kernels - 192 bytes per guide come back
  select   Genome.search_select_classified(top_k=--top-k): search, classify in place, selection, sort of the survivors
  records  the route the library offered before: Genome.search_streamed in batches of --batch reads, Forest.classify_hits per
           batch with the votes copied out (2 bytes per hit), the records copied out (16 bytes per hit) and the same rows and
           top-K reduced on the host with numpy
Per route: the steps' times, vsc_timing's stages (scan_ms, score_ms, sort_ms, finalize_ms; the record route's score_ms is the
sum of its classify kernels), hits per second and the bytes returned to the host.  The rows of the routes are compared.
The activities are drawn from the reference's own 16 TUSCAN values (tests/golden/guides_ontargets.tsv) by guide index.
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
from varscot_amd import _lib, dist as vdist, synth  # noqa: E402
from varscot_amd.classifier import DEFAULT_MODEL, Forest  # noqa: E402

STAGES = ("scan_ms", "score_ms", "sort_ms", "finalize_ms", "total_ms", "hits", "read_passes")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--guides", type=int, default=1000)
    ap.add_argument("--bases", type=int, default=3_000_000_000)
    ap.add_argument("--mismatches", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--top-k", type=int, default=100)
    ap.add_argument("--batch", type=int, default=250, help="record route: reads per streamed batch")
    ap.add_argument("--routes", default="summary,select,records")
    ap.add_argument("--out", help="also write the JSON result to this file")
    args = ap.parse_args()
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    genome.build_index()
    _, seqs = synth.synthetic_guides(args.guides)
    codes = va.pack_guides(seqs)
    forest = Forest(DEFAULT_MODEL)
    golden = os.path.join(ROOT, "tests", "golden", "guides_ontargets.tsv")
    tuscan = [float(line.split("\t")[2]) for line in open(golden) if not line.startswith("#")]
    act = np.array([tuscan[i % len(tuscan)] for i in range(args.guides)], dtype=np.float64)
    m, n_trees = args.mismatches, forest.n_trees

    def summary():
        plain, rows = genome.summarize_classified(codes, m, forest, act, algorithm="seed")
        return dict(rows=rows, bytes=plain.nbytes + rows.nbytes, timing=ctx.timing())

    def select():
        h, plain, rows = genome.search_select_classified(codes, m, forest, act, top_k=args.top_k, algorithm="seed", summary=True)
        n = len(h)
        rec = h.to_numpy().copy()
        h.close()
        return dict(rows=rows, selected=n, top=rec, bytes=plain.nbytes + rows.nbytes + 16 * n, timing=ctx.timing())

    def records():
        rows = np.zeros(args.guides, dtype=_lib.VOTES_DTYPE)
        state = dict(score_ms=0.0, bytes=0, host_ms=0.0, top=[])

        def on_batch(h, first, count):
            if not len(h):
                return
            votes, _ = forest.classify_hits(h, act)
            state["score_ms"] += ctx.timing()["score_ms"]
            rec = h.to_numpy()
            state["bytes"] += rec.nbytes + votes.nbytes
            t0 = time.perf_counter()
            g, v = rec["guide"].astype(np.int64), votes.astype(np.int64)
            active = 2 * v > n_trees
            rows["votes_sum"] += np.bincount(g, weights=v, minlength=args.guides).astype(np.uint64)
            rows["active"] += np.bincount(g[active], minlength=args.guides).astype(np.uint64)
            rows["ties"] += np.bincount(g[2 * v == n_trees], minlength=args.guides).astype(np.uint64)
            nm_of = (rec["info"][active] >> 23) & 31
            rows["active_nm"] += np.bincount(g[active] * 9 + nm_of, minlength=9 * args.guides).reshape(-1, 9).astype(np.uint64)
            # top-K per guide: the records arrive sorted by (guide, strand, global position)
            order = np.lexsort((np.arange(len(g)), -v, g))
            rank = np.arange(len(g)) - np.searchsorted(g[order], g[order], side="left")
            state["top"].append(rec[np.sort(order[rank < args.top_k])].copy())
            state["host_ms"] += (time.perf_counter() - t0) * 1e3

        genome.search_streamed(codes, m, on_batch, batch=args.batch, algorithm="seed")
        t = ctx.timing()
        t["score_ms"] = state["score_ms"]
        return dict(rows=rows, bytes=state["bytes"], host_reduce_ms=state["host_ms"], top=np.concatenate(state["top"]) if state["top"] else None,
                    timing=t)

    routes = {"summary": summary, "select": select, "records": records}
    names = [r for r in args.routes.split(",") if r]
    times = {r: [] for r in names}
    last = {}
    for step in range(args.warmup + args.steps):  # interleaved rounds: every round runs every route once
        for r in names:
            t0 = time.perf_counter()
            last[r] = routes[r]()
            if step >= args.warmup:
                times[r].append((time.perf_counter() - t0) * 1e3)
    res = {"genome_bases": args.bases, "guides": args.guides, "max_mismatches": m, "n_trees": n_trees, "steps": args.steps,
           "warmup": args.warmup, "top_k": args.top_k, "batch": args.batch, "routes": {}}
    for r in names:
        t, ms = last[r]["timing"], times[r]
        hits = int(t["hits"])
        entry = {"ms_per_step": {"mean": sum(ms) / len(ms), "min": min(ms), "max": max(ms), "all": ms},
                 "stages": {k: t[k] for k in STAGES}, "hits_per_s": hits / (sum(ms) / len(ms) / 1e3),
                 "score_ns_per_hit": t["score_ms"] * 1e6 / max(hits, 1), "bytes_returned": int(last[r]["bytes"])}
        for k in ("selected", "host_reduce_ms"):
            if k in last[r]:
                entry[k] = last[r][k]
        res["routes"][r] = entry
    if "records" in last:
        for r in ("summary", "select"):
            if r in last:
                res["routes"][r]["rows_equal_records"] = bool(last[r]["rows"].tobytes() == last["records"]["rows"].tobytes())
                res["routes"][r]["time_vs_records"] = res["routes"][r]["ms_per_step"]["mean"] / res["routes"]["records"]["ms_per_step"]["mean"]
        if "select" in last and last["records"]["top"] is not None:
            res["routes"]["select"]["top_equal_records"] = bool(last["select"]["top"].tobytes() == last["records"]["top"].tobytes())
        ms = res["routes"]["records"]["ms_per_step"]
        res["records_spread"] = (ms["max"] - ms["min"]) / ms["mean"]
    text = json.dumps(res)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()

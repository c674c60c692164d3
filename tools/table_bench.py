"""Per-guide table rows and top-K by table score (vsc_search_summary_table / vsc_search_select_table) against the plain summary
and the record route, on bench.py's synthetic genome (tools/classify_bench.py's) at 8 mismatches, one GPU.

    python tools/table_bench.py --guides 1000 --steps 3 --warmup 1 [--out profiles/table_score.json]

The inputs are made as bench.py makes them (varscot_amd.synth: same contig table, planes and seeds, the first --guides of its
guides; the seed index built before the timed steps).  The table is a seeded random one (weights in (0, 1), 12 of them 0): the
package ships none, and the kernels' work does not depend on the weights' values.  Four routes, timed in interleaved rounds of
one process (W untimed rounds, then K rounds; host wall time per step, every step ends in a device synchronise):
  table    Genome.summarize_table(plain=True): search, table score in place, the two summary kernels - 192 bytes per guide
  select   Genome.search_select_table(top_k=--top-k): search, table score in place, selection, sort of the survivors
  summary  Genome.summarize: search and summary_kernel alone (the MIT rows), for the cost of the table stage beside it
  records  the route the library offered before: Genome.search_streamed in batches of --batch reads, Hits.table_scores per batch
           with the fixed-point words copied out (4 bytes per hit), the records copied out (16 bytes per hit) and the rows
           reduced on the host with numpy
Per route: the steps' times, vsc_timing's stages (scan_ms, score_ms = table_score_kernel, sort_ms, finalize_ms = the summary
kernels), hits per second and the bytes returned.  The rows of the routes are compared; table_score_kernel's time per hit is
reported beside summary_kernel's (the `summary` route's finalize_ms per hit) of the same run.
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

STAGES = ("scan_ms", "score_ms", "sort_ms", "finalize_ms", "total_ms", "hits", "read_passes")


def random_table(seed):
    rng = np.random.default_rng(seed)
    pair = rng.uniform(0.01, 0.99, size=(20, 4, 4))
    off = [(j, g, s) for j in range(20) for g in range(4) for s in range(4) if g != s]
    for k in rng.permutation(len(off))[:12]:
        pair[off[k]] = 0.0
    for b in range(4):
        pair[:, b, b] = 1.0
    return va.ScoreTable(pair, rng.uniform(0.01, 0.99, size=16))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--guides", type=int, default=1000)
    ap.add_argument("--bases", type=int, default=3_000_000_000)
    ap.add_argument("--mismatches", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--top-k", type=int, default=100)
    ap.add_argument("--batch", type=int, default=250, help="record route: reads per streamed batch")
    ap.add_argument("--routes", default="table,select,summary,records")
    ap.add_argument("--out", help="also write the JSON result to this file")
    args = ap.parse_args()
    contigs, _ = synth.contig_table(args.bases)
    span = int(contigs[-1]["offset"]) + int(contigs[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, contigs)
    del hi, lo, nm
    genome.build_index()
    _, seqs = synth.synthetic_guides(args.guides)
    codes = va.pack_guides(seqs)
    table = random_table(4020)
    m = args.mismatches

    def table_route():
        plain, rows = genome.summarize_table(codes, m, table, algorithm="seed", plain=True)
        return dict(rows=rows, bytes=plain.nbytes + rows.nbytes, timing=ctx.timing())

    def select():
        h, rows = genome.search_select_table(codes, m, table, top_k=args.top_k, algorithm="seed", summary=True)
        n = len(h)
        h.close()
        return dict(rows=rows, selected=n, bytes=rows.nbytes + 16 * n, timing=ctx.timing())

    def summary():
        plain = genome.summarize(codes, m, algorithm="seed")
        return dict(bytes=plain.nbytes, timing=ctx.timing())

    def records():
        rows = np.zeros(args.guides, dtype=_lib.TABLE_ROW_DTYPE)
        state = dict(score_ms=0.0, bytes=0, host_ms=0.0)

        def on_batch(h, first, count):
            if not len(h):
                return
            _, f = h.table_scores(table, scores=False)
            state["score_ms"] += ctx.timing()["score_ms"]
            rec = h.to_numpy()
            state["bytes"] += rec.nbytes + f.nbytes
            t0 = time.perf_counter()
            g, pos = rec["guide"].astype(np.int64), f > 0
            rows["score_sum"] += np.bincount(g, weights=f.astype(np.float64), minlength=args.guides).astype(np.uint64)  # (< 2^53: exact)
            rows["positive"] += np.bincount(g[pos], minlength=args.guides).astype(np.uint64)
            nm_of = (rec["info"][pos] >> 23) & 31
            rows["positive_nm"] += np.bincount(g[pos] * 9 + nm_of, minlength=9 * args.guides).reshape(-1, 9).astype(np.uint64)
            state["host_ms"] += (time.perf_counter() - t0) * 1e3

        genome.search_streamed(codes, m, on_batch, batch=args.batch, algorithm="seed")
        t = ctx.timing()
        t["score_ms"] = state["score_ms"]
        return dict(rows=rows, bytes=state["bytes"], host_reduce_ms=state["host_ms"], timing=t)

    routes = {"table": table_route, "select": select, "summary": summary, "records": records}
    names = [r for r in args.routes.split(",") if r]
    times = {r: [] for r in names}
    last = {}
    for step in range(args.warmup + args.steps):  # interleaved rounds: every round runs every route once
        for r in names:
            t0 = time.perf_counter()
            last[r] = routes[r]()
            if step >= args.warmup:
                times[r].append((time.perf_counter() - t0) * 1e3)
    res = {"genome_bases": args.bases, "guides": args.guides, "max_mismatches": m, "steps": args.steps, "warmup": args.warmup,
           "top_k": args.top_k, "batch": args.batch, "routes": {}}
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
    if "table" in last and "summary" in last:  # the two kernels of one run, per hit
        hits = max(int(last["summary"]["timing"]["hits"]), 1)
        res["table_score_kernel_ns_per_hit"] = last["table"]["timing"]["score_ms"] * 1e6 / hits
        res["summary_kernel_ns_per_hit"] = last["summary"]["timing"]["finalize_ms"] * 1e6 / hits
    if "records" in last:
        for r in ("table", "select"):
            if r in last:
                res["routes"][r]["rows_equal_records"] = bool(last[r]["rows"].tobytes() == last["records"]["rows"].tobytes())
                res["routes"][r]["time_vs_records"] = res["routes"][r]["ms_per_step"]["mean"] / res["routes"]["records"]["ms_per_step"]["mean"]
        ms = res["routes"]["records"]["ms_per_step"]
        res["records_spread"] = (ms["max"] - ms["min"]) / ms["mean"]
    text = json.dumps(res)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    table.close()
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()

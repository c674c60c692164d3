"""Table scores of pattern hits (vsc_search_pattern_table) on the synthetic hg38-sized genome of varscot_amd.synth, one GPU -
tools/pattern_bench.py's genome and guides.

    python tools/pattern_table_bench.py                 all cases, JSON to profiles/pattern_table.json (and stdout)
    python tools/pattern_table_bench.py --calls 1 --warmup 0 --routes b --out /tmp/x.json      (what a kernel trace needs)

Per case the routes, interleaved (every round runs each route once), W warm-up rounds, then K timed ones:
    a   search_pattern, rows only                      the unscored search
    b   search_pattern_table, both kinds of rows only  the scored write pass beside it
    c   search_pattern_table, records + f + rows
    d   ... with top_k = 100                           the selection stage behind it
    e   the record route: search_pattern's records copied out, every site read from the host's planes and scored with numpy
        (the same product in the same order: asserted equal to c's f words)
Reported per route: host wall time per call, the kernels' time (vsc_timing.scan_ms) and score_ms (the selection stage),
fastest .. slowest; per case b/a and d/c at the fastest, the records, the longest per-guide segment (records of one guide)
and the selection stage's time for that guide alone.  The cases: pattern_bench's plain23 and Cas12a at m = 4 (few records:
the cost of the scored pass itself) and plain23 at m = 8 (tens of thousands of records per guide: the selection's).
A random table: weights in (0, 1), some exactly 0.
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


def random_table(rng, pattern, protospacer):
    pam_pos = tuple(j for j, ch in enumerate(pattern) if ch != "N")[:4]
    pair = rng.random((protospacer[1], 4, 4))
    pair[rng.random(pair.shape) < 0.05] = 0.0
    for b in range(4):
        pair[:, b, b] = 1.0
    return va.PatternTable(len(pattern), protospacer, pair, pam_pos, rng.random(4 ** len(pam_pos)))


def numpy_scores(rec, guides, table, hi, lo, offsets):
    """f per record from the host's planes: the site's letters gathered bit by bit, the product in the definition's order."""
    L, (start, n) = table.length, table.protospacer
    gpos = offsets[rec["contig"]].astype(np.int64) + rec["pos"].astype(np.int64)
    minus = (rec["info"] >> 31).astype(bool)
    site = np.empty((len(rec), L), dtype=np.int64)
    for j in range(L):
        p = gpos + j
        code = ((hi[p >> 5] >> (p & 31).astype(np.uint32)) & 1).astype(np.int64) * 2 + ((lo[p >> 5] >> (p & 31).astype(np.uint32)) & 1)
        site[:, j] = code
    site[minus] = 3 - site[minus][:, ::-1]
    codes = np.array([["ACGT".find(ch) for ch in g.upper()] for g in guides], dtype=np.int64)[rec["guide"]]  # -1: degenerate
    x = np.ones(len(rec))
    for i in range(n):
        g, s = codes[:, start + i], site[:, start + i]
        x = x * np.where((g >= 0) & (g != s), table.pair[i, np.maximum(g, 0), s], 1.0)
    k = np.zeros(len(rec), dtype=np.int64)
    for q in table.pam_positions:
        k = 4 * k + site[:, q]
    return np.rint(x * table.pam[k] * float(va.TABLE_ONE)).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--guides", type=int, default=16)
    ap.add_argument("--routes", default="a,b,c,d,e")
    ap.add_argument("--cases", default="plain23,Cas12a,plain23_m8")
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pattern_table.json"))
    args = ap.parse_args()
    contigs, _ = synth.contig_table(args.bases)
    span = int(contigs[-1]["offset"]) + int(contigs[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, contigs)
    del nm
    offsets = np.asarray(contigs["offset"], dtype=np.int64)
    guides = list(synth.synthetic_guides(args.guides)[1])
    cas12a, _ = va.pattern_strings("Cas12a")
    cases = {"plain23": ("N" * 21 + "GR", list(guides), 4, (0, 20)),
             "Cas12a": (cas12a, ["N" * 4 + g for g in guides], 4, va.pattern_protospacer("Cas12a")),
             "plain23_m8": ("N" * 21 + "GR", list(guides), 8, (0, 20))}
    routes = args.routes.split(",")
    rng = np.random.default_rng(2022)
    res = {"genome_bases": args.bases, "guides": args.guides, "calls": args.calls, "warmup": args.warmup, "cases": {}}
    for name in args.cases.split(","):
        pattern, gs, m, proto = cases[name]
        table = random_table(rng, pattern, proto)
        state = {}

        def run(route):
            t0 = time.perf_counter()
            if route == "a":
                genome.search_pattern(pattern, gs, m, records=False)
            elif route == "b":
                genome.search_pattern_table(pattern, gs, m, table, records=False)
            elif route == "c":
                state["c"] = genome.search_pattern_table(pattern, gs, m, table)
            elif route == "d":
                state["d"] = genome.search_pattern_table(pattern, gs, m, table, top_k=100)
            t = ctx.timing() if route != "e" else None
            if route == "e":
                rec, _ = genome.search_pattern(pattern, gs, m)
                t = ctx.timing()
                state["e"] = numpy_scores(rec, gs, table, hi, lo, offsets)
            return (time.perf_counter() - t0) * 1e3, t["scan_ms"], t["score_ms"]

        times = {r: [] for r in routes}
        for k in range(args.warmup + args.calls):
            for r in routes:  # interleaved: drift hits every route alike
                got = run(r)
                if k >= args.warmup:
                    times[r].append(got)
        case = {"pattern": pattern, "mismatches": m, "routes": {}}
        for r in routes:
            case["routes"][r] = {"wall_ms": sorted(x[0] for x in times[r]), "kernels_ms": sorted(x[1] for x in times[r]),
                                 "score_ms": sorted(x[2] for x in times[r])}
        fastest = lambda r, what="kernels_ms": case["routes"][r][what][0]
        if "a" in routes and "b" in routes:
            case["b_over_a_kernels"] = fastest("b") / fastest("a")
            case["b_over_a_wall"] = fastest("b", "wall_ms") / fastest("a", "wall_ms")
        if "c" in routes:
            rec, f, rows, trows = state["c"]
            case["records"] = len(rec)
            per_guide = rows.sum(1)
            longest = int(per_guide.argmax())
            case["longest_segment"] = {"guide": longest, "records": int(per_guide[longest])}
            if "d" in routes:
                case["d_over_c_kernels_plus_selection"] = (fastest("d") + fastest("d", "score_ms")) / fastest("c")
                case["d_over_c_wall"] = fastest("d", "wall_ms") / fastest("c", "wall_ms")
                case["records_top_100"] = len(state["d"][0])
                alone = []
                for _ in range(args.calls):
                    genome.search_pattern_table(pattern, [gs[longest]], m, table, top_k=100)
                    alone.append(ctx.timing()["score_ms"])
                case["longest_segment"]["selection_ms"] = sorted(alone)
            if "e" in routes:
                assert state["e"].tobytes() == f.tobytes()  # the record route computes the same words
                case["c_over_e_wall"] = fastest("c", "wall_ms") / fastest("e", "wall_ms")
        res["cases"][name] = case
        print(json.dumps({name: case}), flush=True)
    genome.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

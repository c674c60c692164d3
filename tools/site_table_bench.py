"""Table scores of cut sites (vsc_sites_table) on the synthetic hg38-sized genome of varscot_amd.synth, one GPU -
tools/sites_bench.py's genome and guides.

    python tools/site_table_bench.py                    both cases, JSON to profiles/site_table.json (and stdout)

16 synthetic guides at 4 mismatches, the cases -u 1,1 and -u 2,2, a random SpCas9 bulge table (the package ships none).  One
process; after W warm-up rounds, K rounds that each run every variant once, one after the other (interleaved: a drift of the
machine hits all variants alike); every figure fastest .. slowest:
  stages       the three new stages between HIP events on the context's stream (vsc_debug_site_table_ms): the score kernel,
               the selection's bounds + radix select, its walk (top_k = 100 per guide) - over sites that stay on the device,
               beside the collapse's two stages (vsc_debug_sites_ms) and the bulge search's kernels they follow;
  call         host wall time of the one vsc_sites_table call (records, rows, the read-back that sizes the result);
  unscored     host wall time of Genome.search_sites without a table: the yardstick, the path as it was;
  scored       host wall time of Genome.search_sites(table=...): the same searches and collapse, the sites scored where they
               lie, sites and score records copied out;  scored / unscored is reported per round;
  host route   once per case, not timed per round: the sites copied out and the first --host-sites of them scored member by
               member through vsc_bulge_table_score (the letters decoded from the host planes) - compared with the device's
               score records byte for byte, reported in microseconds per site.
"""
import argparse
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

COMP = str.maketrans("ACGT", "TGCA")


def random_table(seed=7):
    rng = np.random.default_rng(seed)
    pair = rng.random((20, 4, 4))
    for b in range(4):
        pair[:, b, b] = 1.0
    base = va.PatternTable(23, (0, 20), pair, (21, 22), rng.random(16))
    try:
        return va.BulgeTable(base, rng.random((20, 4)), rng.random((20, 4)))
    finally:
        base.close()


def stages_round(ctx, genome, codes, texts, table, m, dna, rna, top_k):
    L = va.lib()
    p = genome._params(m, None, "scan")
    bp = _lib.BulgeParams(dna, rna, 0, 0, 0)
    plain, bulged, sites = C.c_void_p(), C.c_void_p(), C.c_void_p()
    try:
        _lib.check(L.vsc_search(ctx._h, genome._h, _lib.ptr(codes), len(codes), C.byref(p), C.byref(plain)), ctx._h)
        _lib.check(L.vsc_search_bulges(ctx._h, genome._h, _lib.ptr(codes), len(codes), C.byref(p), C.byref(bp), C.byref(bulged), None), ctx._h)
        bulge_ms = ctx.timing()["scan_ms"]
        sp = _lib.SiteParams(23, _lib.SITE_ANCHOR_END)
        _lib.check(L.vsc_hits_sites(ctx._h, plain, bulged, len(codes), C.byref(sp), C.byref(sites), None), ctx._h)
        flag, write = C.c_double(0), C.c_double(0)
        _lib.check(L.vsc_debug_sites_ms(ctx._h, C.byref(flag), C.byref(write)), ctx._h)
        t0 = time.perf_counter()
        rec, scores, rows = genome._site_scores(sites, sp, texts, table, top_k, 0, True, True)
        wall = (time.perf_counter() - t0) * 1e3
        score, select, walk = C.c_double(0), C.c_double(0), C.c_double(0)
        _lib.check(L.vsc_debug_site_table_ms(ctx._h, C.byref(score), C.byref(select), C.byref(walk)), ctx._h)
        return {"score_ms": score.value, "select_ms": select.value, "walk_ms": walk.value, "call_wall_ms": wall, "collapse_flag_scan_ms": flag.value,
                "collapse_write_ms": write.value, "bulge_search_kernels_ms": bulge_ms, "sites": int(L.vsc_sites_count(sites)), "kept": len(rec),
                "positive": int(rows["positive"].sum())}
    finally:
        L.vsc_sites_free(sites)
        L.vsc_bulge_hits_free(bulged)
        L.vsc_hits_free(plain)


def letters(hi, lo, start, n):
    idx = start + np.arange(n, dtype=np.int64)
    w, b = idx >> 5, (idx & 31).astype(np.uint32)
    code = (((hi[w] >> b) & 1) << 1 | ((lo[w] >> b) & 1)).astype(np.intp)
    return np.frombuffer(b"ACGT", dtype=np.uint8)[code].tobytes().decode()


def host_route(hi, lo, contig_off, sites, scores, texts, table, limit):
    """vsc_bulge_table_score member by member over the first `limit` sites; (microseconds per site, sites compared)"""
    n = min(limit, len(sites))
    t0 = time.perf_counter()
    for k in range(n):
        s = sites[k]
        strand, info = int(s["info"]) >> 31, int(s["info"])
        best_d = (-1 if (info >> 12) & 1 else 1) * ((info >> 10) & 3)
        at_start = strand == 1  # the END anchor: the members share pos on '-'
        best = top = top_d = top_rank = None
        for d in range(-2, 3):
            if (int(s["members"]) >> (5 * (d + 2))) & 31 == 31:
                continue
            pos = int(s["anchor"]) if at_start else int(s["anchor"]) - (23 + d)
            text = letters(hi, lo, contig_off[int(s["contig"])] + pos, 23 + d)
            if strand:
                text = text.translate(COMP)[::-1]
            nm, _, _, f = table.score(texts[int(s["guide"])], text, d, fixed=True)
            rank = (nm + abs(d), abs(d), d < 0)
            if d == best_d:
                best = f
            if top is None or f > top or (f == top and rank < top_rank):
                top, top_d, top_rank = f, d + 2, rank
        assert (best, top, top_d) == (int(scores["best"][k]), int(scores["top"][k]), int(scores["top_d"][k])), k
    return (time.perf_counter() - t0) * 1e6 / max(n, 1), n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--guides", type=int, default=16)
    ap.add_argument("--mismatches", type=int, default=4)
    ap.add_argument("--top-k", type=int, default=100)
    ap.add_argument("--host-sites", type=int, default=5000)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "site_table.json"))
    args = ap.parse_args()
    contigs, _ = synth.contig_table(args.bases)
    span = int(contigs[-1]["offset"]) + int(contigs[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, contigs)
    del nm
    contig_off = [int(c["offset"]) for c in contigs]
    codes = va.pack_guides(synth.synthetic_guides(args.guides)[1])
    texts = [t.encode() for t in va.unpack_guides(codes)]
    table = random_table()
    m = args.mismatches
    res = {"genome_bases": args.bases, "guides": args.guides, "mismatches": m, "calls": args.calls, "warmup": args.warmup, "top_k": args.top_k,
           "cases": {}}
    for dna, rna in ((1, 1), (2, 2)):
        rounds = []
        for r in range(args.warmup + args.calls):
            one = stages_round(ctx, genome, codes, texts, table, m, dna, rna, args.top_k)
            t0 = time.perf_counter()
            plain = genome.search_sites(codes, m, dna=dna, rna=rna, algorithm="scan")
            t1 = time.perf_counter()
            scored = genome.search_sites(codes, m, dna=dna, rna=rna, algorithm="scan", table=table)
            t2 = time.perf_counter()
            assert scored[0].tobytes() == plain[0].tobytes() and scored[1].tobytes() == plain[1].tobytes()
            one["unscored_wall_ms"], one["scored_wall_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
            one["scored_over_unscored"] = one["scored_wall_ms"] / one["unscored_wall_ms"]
            if r >= args.warmup:
                rounds.append(one)
        per_site_us, compared = host_route(hi, lo, contig_off, scored[0], scored[2], [t.decode() for t in texts], table, args.host_sites)
        case = {k: rounds[0][k] for k in ("sites", "kept", "positive")}
        for k in ("score_ms", "select_ms", "walk_ms", "call_wall_ms", "collapse_flag_scan_ms", "collapse_write_ms", "bulge_search_kernels_ms",
                  "unscored_wall_ms", "scored_wall_ms", "scored_over_unscored"):
            case[k] = sorted(r[k] for r in rounds)
        case["host_route_us_per_site"], case["host_route_sites_compared"] = per_site_us, compared
        case["host_route_all_sites_ms_extrapolated"] = per_site_us * case["sites"] / 1e3
        res["cases"]["u%d,%d" % (dna, rna)] = case
        print(json.dumps({"u%d,%d" % (dna, rna): case}), flush=True)
    table.close()
    genome.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""The paired-nickase join (vsc_hits_pairs) against the record route it replaces, on bench.py's synthetic genome, one GPU.

    python tools/pairs_bench.py --steps 3 --warmup 1          one JSON line on stdout, the same into profiles/pairs_bench.json

The genome is made as bench.py makes it (varscot_amd.synth: same contig table, planes and seed; the seed index built before
anything is timed).  The guides are the candidates the device finds in one target interval of --target-bases bases (a few
thousand: vsc_guides_enumerate), the pairs all PAM-out pairs among them with a nickase offset of --offset (vsc_guides_pairs),
the records those of one search of the guides at <= --mismatches mismatches.  Two routes from the resident records to the pairs'
rows (sites, nm_sum, nm_max, on_target), each with the guide's own locus excluded:
  join     Hits.pairs(pairs, delta, exclude=loci) - segment table, count pass, rows to the host - between two HIP events on the
           context's stream; also with sites=True (count, scan, write, sites to the host), max_sites sized from the rows
  records  Hits.to_numpy() - all records to the host - and a numpy join per pair: the two guides' record blocks, one outer
           difference, the strand / contig / range test, two bincounts; host wall time, the copy and the join apart
The two routes' rows are compared before anything is reported."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import varscot_amd as va  # noqa: E402
from varscot_amd import dist as vdist, synth  # noqa: E402


def numpy_rows(rec, pairs, delta, loci):
    """The rows of vsc_hits_pairs from the records on the host: per pair one outer difference over the two guides' blocks."""
    rows = np.zeros(len(pairs), dtype=va.PAIR_SUMMARY_DTYPE)
    guide = rec["guide"]
    n_guides = len(loci)
    start = np.searchsorted(guide, np.arange(n_guides + 1))
    contig = rec["contig"].astype(np.int64)
    pos = rec["pos"].astype(np.int64)
    strand = (rec["info"] >> 31).astype(np.int64)
    nm = ((rec["info"] >> 23) & 31).astype(np.int64)
    for j, (a, b) in enumerate(pairs):
        sa, sb = slice(start[a], start[a + 1]), slice(start[b], start[b + 1])
        d = np.where(strand[sa][:, None] == 0, pos[sa][:, None] - pos[sb][None, :], pos[sb][None, :] - pos[sa][:, None])
        ok = (contig[sa][:, None] == contig[sb][None, :]) & (strand[sa][:, None] != strand[sb][None, :]) & (d >= delta[0]) & (d <= delta[1])
        at_a = (contig[sa] == loci["contig"][a]) & (pos[sa] == loci["pos"][a]) & (strand[sa] == loci["strand"][a])
        at_b = (contig[sb] == loci["contig"][b]) & (pos[sb] == loci["pos"][b]) & (strand[sb] == loci["strand"][b])
        on = ok & at_a[:, None] & at_b[None, :]
        rows["on_target"][j] = int(on.any())
        x, y = np.nonzero(ok & ~on)
        na, nb = nm[sa][x], nm[sb][y]
        rows["sites"][j] = len(x)
        rows["nm_sum"][j] = np.bincount(na + nb, minlength=17)[:17]
        rows["nm_max"][j] = np.bincount(np.maximum(na, nb), minlength=9)[:9]
    return rows


def stats(ms):
    return {"mean": sum(ms) / len(ms), "min": min(ms), "max": max(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="synthetic genome size (bench.py: 3 000 000 000)")
    ap.add_argument("--target-bases", type=int, default=25_000, help="length of the target interval the guides are found in")
    ap.add_argument("--mismatches", type=int, default=4)
    ap.add_argument("--offset", type=lambda t: tuple(int(x) for x in t.split(",")), default=(-4, 20), metavar="MIN,MAX")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_bench.json"))
    args = ap.parse_args()
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    genome.build_index()
    t0 = int(table[0]["length"]) // 3
    regions = va.Regions(va.PackedGenome(None, None, None, table), [(0, t0, t0 + args.target_bases)], rule="inside")
    delta = va.nickase_delta(*args.offset)
    codes, loci, pairs = genome.enumerate_pairs(delta, regions)
    hits = genome.search(codes, args.mismatches, algorithm="seed")
    res = {"genome_bases": args.bases, "guides": len(codes), "pairs": len(pairs), "max_mismatches": args.mismatches,
           "offset": list(args.offset), "delta": list(delta), "records": len(hits), "record_bytes": 16 * len(hits),
           "steps": args.steps, "warmup": args.warmup}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ev, wall, out = [], [], None
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            e0.record(stream)
            out = fn()
            e1.record(stream)
            e1.synchronize()
            wall.append((time.perf_counter() - w0) * 1e3)
            ev.append(e0.elapsed_time(e1))
        return {"event_ms": stats(ev), "wall_ms": stats(wall)}, out

    t_rows, rows = timed(lambda: hits.pairs(pairs, delta, exclude=loci))
    total = int(rows["sites"].sum())
    t_sites, both = timed(lambda: hits.pairs(pairs, delta, exclude=loci, sites=True, max_sites=max(total, 1)))
    res["join"] = {"rows": t_rows, "rows_and_sites": t_sites, "sites": total, "on_targets": int(rows["on_target"].sum()),
                   "work_items": int(sum(np.bincount(hits.to_numpy()["guide"], minlength=len(codes))[pairs[:, 0]]))}
    # the record route: the copy (a fresh result each step: the host copy of a result is kept once made), then the join
    copy_ms, join_ms, want = [], [], None
    for step in range(args.warmup + args.steps):
        h = genome.search(codes, args.mismatches, algorithm="seed")
        w0 = time.perf_counter()
        rec = h.to_numpy()
        w1 = time.perf_counter()
        want = numpy_rows(rec, pairs.tolist(), delta, loci)
        w2 = time.perf_counter()
        h.close()
        if step >= args.warmup:
            copy_ms.append((w1 - w0) * 1e3)
            join_ms.append((w2 - w1) * 1e3)
    res["records_route"] = {"copy_ms": stats(copy_ms), "numpy_join_ms": stats(join_ms),
                            "total_ms": stats([c + j for c, j in zip(copy_ms, join_ms)])}
    res["same_rows"] = bool(want.tobytes() == rows.tobytes() and both[0].tobytes() == rows.tobytes() and len(both[1]) == total)
    res["join_vs_copy"] = t_rows["event_ms"]["mean"] / res["records_route"]["copy_ms"]["mean"]
    res["join_vs_records_route"] = t_rows["event_ms"]["mean"] / res["records_route"]["total_ms"]["mean"]
    text = json.dumps(res)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    hits.close()
    regions.close()
    genome.close()
    ctx.close()
    return 0 if res["same_rows"] else 1


if __name__ == "__main__":
    sys.exit(main())

"""The variant-aware pattern screen (vsc_search_pattern_variants) against its parts and against the record route, one GPU.

    python tools/pattern_variants_bench.py                                 JSON to profiles/pattern_variants.json (and stdout)
    python tools/pattern_variants_bench.py --bases 300000000 --snps 300000 --out /tmp/x.json     a tenth of the size

The synthetic hg38-sized genome and VCF of varscot_amd.synth (the other tools' inputs), the windows built with seq_len = 27,
SaCas9 (N x 21 + NNGRRT, L = 27), 16 synthetic guides (their first 21 letters + N x 6), m = 4.  Per route W warm-up calls, then
K timed calls, host wall time per call, fastest .. slowest (the spread is what the list shows):
  searches  vsc_search_pattern on the reference and on the window genome, the records kept on the device and freed: what the
            screen cannot go below
  screen    vsc_search_pattern_variants: the same two searches, both merge kernels, six row arrays back.  merge_kernels_ms is
            vsc_ctx_timing's finalize_ms (HIP events around the two kernels), kernels_ms its total_ms
  records   the record route: both searches, both results copied to the host and merged there with numpy - the shadow test by
            a binary search over the windows' intervals (parsed from the ids once, outside the timed calls), the walk of
            every window record by VariantMap.locate / .tag, the neighbour rule on the keys.  Its rows must equal the screen's
            (same_rows)
No kernel trace is taken here.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import varscot_amd as va  # noqa: E402
from varscot_amd import synth  # noqa: E402

L = 27
PATTERN = "N" * 21 + "NNGRRT"


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms, out = [], None
    for _ in range(calls):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms), out


def shadow_intervals(win, names, full):
    """(start[], end_max[]) of the windows' intervals in the reference's global positions, sorted by start."""
    chrom = {n.split()[0]: c for c, n in reversed(list(enumerate(full.names)))}
    iv = []
    for wid, length in zip(names, win.contigs["length"]):
        f = wid.split("_")
        if f[0] in chrom and not f[1].startswith("-"):
            c = chrom[f[0]]
            s = int(full.contigs["offset"][c]) + int(f[1])
            iv.append((s, min(s + int(length), int(full.contigs["offset"][c]) + int(full.contigs["length"][c]))))
    iv.sort()
    start = np.array([a for a, _ in iv], dtype=np.int64)
    return start, (np.maximum.accumulate(np.array([b for _, b in iv], dtype=np.int64)) if iv else np.zeros(0, dtype=np.int64))


def host_merge(ref_rec, win_rec, win, names, intervals, vmap, full, n_guides):
    """The mergers on the host over the copied records: (reference counts, window counts, shadowed, duplicates) per guide."""
    ref_count, win_count = np.zeros((n_guides, 9), dtype=np.int64), np.zeros((n_guides, 9), dtype=np.int64)
    # reference side: inside one window's interval <=> the running maximum of the ends of the intervals that start at or
    # before the site reaches the site's end
    start, end_max = intervals
    g = full.contigs["offset"][ref_rec["contig"]].astype(np.int64) + ref_rec["pos"]
    n = np.searchsorted(start, g, side="right")
    shadowed = (n > 0) & (end_max[np.maximum(n, 1) - 1] >= g + L) if len(start) else np.zeros(len(g), dtype=bool)
    np.add.at(ref_count, (ref_rec["guide"][~shadowed], (ref_rec["info"][~shadowed] & 63)), 1)
    # window side: the walk per record, then the neighbour rule on (guide, chr, pos2, strand and NM, mask, tag, bases)
    keys, dups = [], np.zeros(n_guides, dtype=np.int64)
    for i, r in enumerate(win_rec):
        w, p = int(r["contig"]), int(r["pos"])
        lab = vmap.locate(w, p, L)
        off = int(win.contigs["offset"][w]) + p
        keys.append((int(r["guide"]), names[w].split("_")[0], int(lab["pos"]), int(r["info"]), int(r["mask"]), vmap.tag(w, p, L), win.decode(off, L)))
        if i > 0 and keys[i] == keys[i - 1]:
            dups[int(r["guide"])] += 1
        else:
            win_count[int(r["guide"]), int(r["info"]) & 63] += 1
    return ref_count, win_count, np.bincount(ref_rec["guide"][shadowed], minlength=n_guides), dups


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--guides", type=int, default=16)
    ap.add_argument("--bases", type=int, default=3_000_000_000)
    ap.add_argument("--snps", type=int, default=3_000_000)
    ap.add_argument("--mismatches", type=int, default=4)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pattern_variants.json"))
    args = ap.parse_args()

    full = synth.synthetic_genome(args.bases)
    tmp = tempfile.mkdtemp(prefix="vsc_pattern_variants_")
    try:
        n_snps = synth.synthetic_vcf(full, args.snps, os.path.join(tmp, "in.vcf"))
        t0 = time.perf_counter()
        win = va.variant_windows(full, os.path.join(tmp, "in.vcf"), sample=0, seq_len=L)
        t_windows = time.perf_counter() - t0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    t0 = time.perf_counter()
    vmap = va.VariantMap(win, full)
    t_map = time.perf_counter() - t0
    ctx = va.Context(0)
    genome, win_genome = ctx.load_genome(full), ctx.load_genome(win)
    info = vmap.info()
    _, seqs = synth.synthetic_guides(args.guides)
    guides = [g[:21] + "N" * 6 for g in seqs]
    m = args.mismatches
    res = {"pattern": PATTERN, "length": L, "guides": args.guides, "max_mismatches": m, "genome_bases": args.bases, "snps": n_snps,
           "windows": info["windows"], "window_bases": win.n_bases, "map": info, "windows_build_s": t_windows, "map_build_s": t_map,
           "calls": args.calls, "warmup": args.warmup}

    t0 = time.perf_counter()
    names = list(win.names)
    intervals = shadow_intervals(win, names, full)  # (made once, as the map is: the record route's share of the preparation)
    res["host_intervals_s"] = time.perf_counter() - t0

    def searches():
        kernels, n = 0.0, 0
        for gen in (genome, win_genome):
            h = gen.search_pattern_hits(PATTERN, guides, m)
            kernels += ctx.timing()["total_ms"]
            n += len(h)
            h.close()
        return kernels, n

    def screen():
        rows = va.pattern_variants_screen(genome, win_genome, vmap, PATTERN, guides, m)
        return rows, ctx.timing()

    def records():
        out = []
        for gen in (genome, win_genome):
            h = gen.search_pattern_hits(PATTERN, guides, m)
            out.append(h.to_numpy())
            h.close()
        return host_merge(out[0], out[1], win, names, intervals, vmap, full, args.guides), len(out[0]), len(out[1])

    ms, (kernels_ms, n_rec) = timed(searches, args.calls, args.warmup)
    res["searches"] = {"wall_ms": ms, "kernels_ms": kernels_ms, "records": n_rec}
    ms, (rows, t) = timed(screen, args.calls, args.warmup)
    res["screen"] = {"wall_ms": ms, "kernels_ms": t["total_ms"], "merge_kernels_ms": t["finalize_ms"], "search_kernels_ms": t["scan_ms"],
                     "merge_share_of_kernels": t["finalize_ms"] / t["total_ms"] if t["total_ms"] else None, "records": t["hits"],
                     "reference_counted": int(rows["ref"]["count"].sum()), "reference_shadowed": int(rows["ref"]["dropped"].sum()),
                     "window_counted": int(rows["win"]["count"].sum()), "window_duplicates": int(rows["win"]["dropped"].sum()),
                     "window_var": int(rows["var"]["count"].sum())}
    ms, ((ref_count, win_count, shadowed, dups), n_ref, n_win) = timed(records, args.calls, args.warmup)
    res["records"] = {"wall_ms": ms, "reference_records": n_ref, "window_records": n_win, "bytes_to_host": 20 * (n_ref + n_win)}
    res["same_rows"] = bool(np.array_equal(ref_count, rows["ref"]["count"]) and np.array_equal(win_count, rows["win"]["count"]) and
                            np.array_equal(shadowed, rows["ref"]["dropped"]) and np.array_equal(dups, rows["win"]["dropped"]))
    res["screen_vs_searches"] = res["screen"]["wall_ms"][0] / res["searches"]["wall_ms"][0]
    res["screen_vs_records"] = res["screen"]["wall_ms"][0] / res["records"]["wall_ms"][0]
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res), flush=True)
    vmap.close()
    win_genome.close()
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()

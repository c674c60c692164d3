"""The variant-aware screen (vsc_search_summary_variants) against the record route, on bench.py's c4-shaped workload, one GPU.

    python tools/variants_bench.py --steps 3 --warmup 1                 one JSON line on stdout
    python tools/variants_bench.py --bases 300000000 --snps 500000      the same shape at a tenth of the size

The inputs are made as bench.py makes workload c4 (varscot_amd.synth: contig table, planes, guides, synthetic VCF and their
seeds; the windows by vsc_windows_build; both seed indexes built before the timed steps), and a step is timed as
tools/select_bench.py times it: W untimed steps, then K steps, host wall time per step (mean, fastest and slowest step).
  screen   Genome.summarize(guides, M, regions=shadow) on the reference + Genome.summarize_variants(guides, M, vmap) on the
           window genome: 2 x 96 bytes per guide and the duplicate counts come back, no record leaves the device
  records  Genome.search on both genomes and both results copied to the host (Hits.to_numpy): what varscot_pipeline and
           bam_merger do BEFORE their host loop over the records (tools/varscot_pipeline.cpp:318-330: split_id, snp_type and
           the key comparison per window hit, the shadow test per reference hit).  That loop is not run here, so the record
           route's time is a lower bound and screen_vs_records an upper bound of the ratio.
merge_kernel: the variant_merge_kernel alone (vsc_ctx_timing's finalize_ms of the window screen: HIP events around the
kernel, summed over the batches), its share of the screen's device time, and the record bytes it reads per second (16 bytes
per window hit; the map's tables - map_bytes - are read through the cache).
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

import varscot_amd as va  # noqa: E402
from varscot_amd import synth  # noqa: E402

SPLIT = ("scan_ms", "prep_ms", "sort_ms", "finalize_ms", "total_ms", "hits", "passes", "read_passes", "algorithm")


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"mean": sum(ms) / len(ms), "min": min(ms), "max": max(ms)}, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--guides", type=int, default=1_000)
    ap.add_argument("--bases", type=int, default=3_000_000_000)
    ap.add_argument("--snps", type=int, default=5_000_000)
    ap.add_argument("--mismatches", type=int, default=6)
    ap.add_argument("--batch", type=int, default=0, help="guides per pass of the window screen (0: the default pass size)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--screen-only", action="store_true", help="time the screen only (what a kernel trace needs)")
    args = ap.parse_args()

    full = synth.synthetic_genome(args.bases)
    tmp = tempfile.mkdtemp(prefix="vsc_variants_")
    try:
        n_snps = synth.synthetic_vcf(full, args.snps, os.path.join(tmp, "in.vcf"))
        t0 = time.perf_counter()
        win = va.variant_windows(full, os.path.join(tmp, "in.vcf"), sample=0)
        t_windows = time.perf_counter() - t0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    t0 = time.perf_counter()
    vmap = va.VariantMap(win, full)
    shadow = vmap.shadow()
    t_map = time.perf_counter() - t0
    ctx = va.Context(0)
    genome, win_genome = ctx.load_genome(full), ctx.load_genome(win)
    genome.build_index()
    win_genome.build_index()
    info = vmap.info()
    res = {"workload": "c4", "guides": args.guides, "max_mismatches": args.mismatches, "genome_bases": args.bases, "snps": n_snps,
           "windows": info["windows"], "window_bases": win.n_bases, "map": info, "map_bytes": 16 * (info["windows"] + 1 + info["variants"]),
           "shadow": shadow.info(), "windows_build_s": t_windows, "map_build_s": t_map, "steps": args.steps, "warmup": args.warmup}
    del full, win
    _, seqs = synth.synthetic_guides(args.guides)
    codes = va.pack_guides(seqs)
    split = {}

    def screen():
        ref_all, ref_in = genome.summarize(codes, args.mismatches, algorithm="seed", regions=shadow)
        split["reference"] = ctx.timing()
        win_all, win_var, dups = win_genome.summarize_variants(codes, args.mismatches, vmap, batch=args.batch, algorithm="seed")
        split["windows"] = ctx.timing()
        ind = va.individual_rows(ref_all, ref_in, win_all)
        return int(ind["nm"].sum()), int(win_var["nm"].sum()), int(dups.sum()), int(ref_in["nm"].sum())

    ctx.release_scratch()
    ms, (n_ind, n_var, n_dup, n_shadowed) = timed(screen, args.steps, args.warmup)
    ref_t, win_t = split["reference"], split["windows"]
    device_ms = ref_t["total_ms"] + win_t["total_ms"]
    kernel_ms, win_hits = win_t["finalize_ms"], win_t["hits"]
    res["screen"] = {"ms_per_step": ms, "individual_hits": n_ind, "var_hits": n_var, "duplicates": n_dup, "shadowed_reference_hits": n_shadowed,
                     "reference_timing": {f: ref_t[f] for f in SPLIT}, "window_timing": {f: win_t[f] for f in SPLIT}}
    res["merge_kernel"] = {"ms": kernel_ms, "window_hits": win_hits, "share_of_screen_device_time": kernel_ms / device_ms if device_ms else None,
                           "record_bytes_per_hit": 16, "record_gb_per_s": 16 * win_hits / (kernel_ms * 1e6) if kernel_ms else None,
                           "ns_per_hit": kernel_ms * 1e6 / win_hits if win_hits else None}
    if not args.screen_only:
        def records():
            h_ref = genome.search(codes, args.mismatches, algorithm="seed")
            t_ref = ctx.timing()
            h_win = win_genome.search(codes, args.mismatches, algorithm="seed")
            t_win = ctx.timing()
            n = len(h_ref.to_numpy()) + len(h_win.to_numpy())
            h_ref.close()
            h_win.close()
            return n, t_ref, t_win

        ctx.release_scratch()
        ms_r, (n_rec, t_ref, t_win) = timed(records, args.steps, args.warmup)
        res["records"] = {"ms_per_step": ms_r, "records": n_rec, "bytes_to_host": 16 * n_rec, "host_loop": "not run: lower bound of the record route",
                          "reference_timing": {f: t_ref[f] for f in SPLIT}, "window_timing": {f: t_win[f] for f in SPLIT}}
        res["same_window_hits"] = t_win["hits"] == win_hits
        res["screen_vs_records"] = ms["mean"] / ms_r["mean"]
    print(json.dumps(res), flush=True)
    shadow.close()
    vmap.close()
    win_genome.close()
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()

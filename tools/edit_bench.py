"""Base-editor windows of candidate guides (vsc_guides_edit, vsc_guides_filter_edit) on the synthetic hg38-sized genome of
varscot_amd.synth, one GPU, beside the enumeration that produces the candidates and the microhomology kernel at F = 8 over the
same candidates, in one run and one process.

    python tools/edit_bench.py                      JSON to profiles/edit.json (and stdout)
    python tools/edit_bench.py --calls 1 --warmup 1 (what a kernel trace needs: run it under rocprofv3 --kernel-trace --stats)

Steps (each under its own time limit, --step-seconds: W warm-up calls, then K timed calls, fastest .. slowest)
  enumerate   vsc_guides_enumerate alone: NGG, both strands, no filter, no regions - the yardstick; kernels' time =
              vsc_timing.scan_ms (count pass + scan, write pass)
  mh_f8       + vsc_guides_microhomology at F = 8 over those candidates - the other yardstick
  rows_none   + vsc_guides_edit, window (3, 5), base C, no targets: edit_rows_kernel = vsc_timing.score_ms
  rows_1e6    the same with 10^6 random targets; pairs counted only: the rows kernel, and the pairs' count pass + scan + write
              pass (for the coverage) = vsc_timing.scan_ms
  rows_exons  the same with every C and G of the 250 000 exon-like intervals (synth.synthetic_regions, 3 % of the genome)
  pairs_1e6 / pairs_exons   the same calls with the pairs written and copied to the host
  filter      vsc_guides_filter_edit, 1 .. 16 editable bases, the 10^6 targets: both passes and the scan = vsc_timing.score_ms
  host        the host route over the first --host-candidates candidates: copy the loci out, window starts in numpy,
              numpy.searchsorted into the 10^6 targets; scaled to all candidates beside it
Reported beside each kernel time, the floors DERIVED from the shapes: 24 bytes per candidate (16 of locus read, 8
of row written) for the rows kernel, 8 bytes per candidate + 16 per pair for each pairs pass, at the 6.3 TB/s a float4 copy
kernel reaches."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import varscot_amd as va  # noqa: E402
from varscot_amd import _lib, dist as vdist, synth  # noqa: E402
from varscot_amd.api import _enum_params  # noqa: E402
from efficiency_bench import FLOAT4_COPY_TBS, enumerate_once  # noqa: E402
from microhomology_bench import step_limit  # noqa: E402


def targets_of_global(table, g):
    """EDIT_TARGET_DTYPE (strictly ascending) of sorted distinct global positions g that lie inside contigs."""
    off = np.asarray(table["offset"], dtype=np.int64)
    c = np.searchsorted(off, g, side="right") - 1
    pos = g - off[c]
    ok = pos < np.asarray(table["length"], dtype=np.int64)[c]
    out = np.zeros(int(ok.sum()), dtype=va.EDIT_TARGET_DTYPE)
    out["contig"], out["pos"] = c[ok], pos[ok]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--random-targets", type=int, default=1_000_000)
    ap.add_argument("--intervals", type=int, default=250_000)
    ap.add_argument("--fraction", type=float, default=0.03)
    ap.add_argument("--host-candidates", type=int, default=1 << 24)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit.json"))
    args = ap.parse_args()
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    print(json.dumps({"planes_words": int(len(hi))}), flush=True)
    # the target sets, on the host: random positions; every C and G (hi != lo) of the exon-like intervals
    rng = np.random.default_rng(28)
    random_targets = targets_of_global(table, np.unique(rng.integers(0, span, size=args.random_targets, dtype=np.int64)))
    iv = synth.synthetic_regions(table, args.intervals, args.fraction)
    start = np.asarray(table["offset"], dtype=np.int64)[iv["contig"]] + iv["start"].astype(np.int64)
    length = (iv["end"].astype(np.int64) - iv["start"].astype(np.int64))
    g = np.repeat(start - np.concatenate(([0], np.cumsum(length)[:-1])), length) + np.arange(int(length.sum()), dtype=np.int64)
    g = np.unique(g)
    word, bit = g >> 5, (g & 31).astype(np.uint32)
    cg = (((hi[word] ^ lo[word]) & ~nm[word]) >> bit) & 1
    exon_targets = targets_of_global(table, g[cg.astype(bool)])
    del g, word, bit, cg
    print(json.dumps({"random_targets": len(random_targets), "exon_targets": len(exon_targets)}), flush=True)
    with step_limit("load", args.step_seconds):
        ctx = va.Context(0)
        genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    L = va.lib()
    params = _enum_params("GG", "both", (0, 0), 0, 0)
    res = {"genome_bases": args.bases, "calls": args.calls, "warmup": args.warmup, "float4_copy_tbs": FLOAT4_COPY_TBS,
           "random_targets": len(random_targets), "exon_targets": len(exon_targets)}

    def report(key, value):
        res[key] = value
        print(json.dumps({key: value}), flush=True)
        with open(args.out, "w") as f:  # (what was measured before a step's limit ends the process is in the file)
            json.dump(res, f, indent=1)
            f.write("\n")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        return [fn() for _ in range(args.calls)]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with step_limit("enumerate", args.step_seconds):
        runs = timed(lambda: enumerate_once(ctx, genome, params))
        n = runs[0][2]
        report("enumerate", {"candidates": n, "kernels_ms": sorted(r[1] for r in runs), "wall_ms": sorted(r[0] for r in runs)})
        _, _, _, h = enumerate_once(ctx, genome, params, keep=True)
    enum_ms = res["enumerate"]["kernels_ms"][0]
    rows = np.empty((n, 2), dtype=np.uint32)

    with step_limit("mh_f8", args.step_seconds):
        mh = _lib.MhShape(23, 17, 8, 0)

        def mh_once():
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_microhomology(ctx._h, genome._h, h, C.byref(mh), _lib.ptr(rows), None), ctx._h)
            return (time.perf_counter() - t0) * 1e3, ctx.timing()["score_ms"]

        runs = timed(mh_once)
        report("mh_f8", {"candidates": n, "kernel_ms": sorted(r[1] for r in runs), "wall_ms": sorted(r[0] for r in runs)})
    mh_ms = res["mh_f8"]["kernel_ms"][0]

    shape = va.EDITORS["CBE"]._struct()
    st, count = _lib.EditStats(), C.c_uint64()
    hbm_rows_ms = 24.0 * n / (FLOAT4_COPY_TBS * 1e12) * 1e3

    def edit_step(name, targets, write_pairs):
        with step_limit(name, args.step_seconds):
            n_t = 0 if targets is None else len(targets)
            pairs = None
            if write_pairs:
                _lib.check(L.vsc_guides_edit(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(targets), n_t, None, None, 0, C.byref(count), None,
                                             None), ctx._h)
                pairs = np.empty(int(count.value), dtype=va.EDIT_PAIR_DTYPE)

            def once():
                t0 = time.perf_counter()
                _lib.check(L.vsc_guides_edit(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(targets) if n_t else None, n_t, _lib.ptr(rows),
                                             _lib.ptr(pairs), 0 if pairs is None else len(pairs), C.byref(count), None, C.byref(st)), ctx._h)
                wall = (time.perf_counter() - t0) * 1e3
                t = ctx.timing()
                return wall, t["score_ms"], t["scan_ms"]

            runs = timed(once)
            kernel = sorted(r[1] for r in runs)
            out = {"candidates": n, "targets": n_t, "stats": st.as_dict(), "rows_kernel_ms": kernel, "wall_ms": sorted(r[0] for r in runs),
                   "rows_floor_hbm_ms": hbm_rows_ms, "rows_kernel_over_enumerate_kernels": kernel[0] / enum_ms,
                   "rows_kernel_over_mh_f8_kernel": kernel[0] / mh_ms}
            if n_t:
                # count pass: 8 B per candidate; write pass: 8 B per candidate + 16 B per pair (written only with write_pairs)
                pass_bytes = 16.0 * n + (16.0 * st.pairs if write_pairs else 0.0)
                out.update(pairs_passes_ms=sorted(r[2] for r in runs), pairs_written=bool(write_pairs),
                           pairs_floor_hbm_ms=pass_bytes / (FLOAT4_COPY_TBS * 1e12) * 1e3)
            report(name, out)

    edit_step("rows_none", None, False)
    edit_step("rows_1e6", random_targets, False)
    edit_step("rows_exons", exon_targets, False)
    edit_step("pairs_1e6", random_targets, True)
    edit_step("pairs_exons", exon_targets, True)

    with step_limit("filter", args.step_seconds):
        def filter_once():
            out = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_filter_edit(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(random_targets), len(random_targets), 1, 16,
                                                C.byref(out)), ctx._h)
            wall = (time.perf_counter() - t0) * 1e3
            kept = int(L.vsc_guides_count(out))
            L.vsc_guides_free(out)
            t = ctx.timing()
            return wall, t["score_ms"], kept, t["genome_bytes"]

        runs = timed(filter_once)
        assert runs[0][2] == res["rows_1e6"]["stats"]["with_hit"], (runs[0][2], res["rows_1e6"]["stats"]["with_hit"])
        report("filter", {"candidates": n, "targets": len(random_targets), "survivors": runs[0][2], "kernels_ms": sorted(r[1] for r in runs),
                          "wall_ms": sorted(r[0] for r in runs), "bytes": runs[0][3],
                          "floor_ms_at_float4_copy_kernel": runs[0][3] / (FLOAT4_COPY_TBS * 1e12) * 1e3})

    with step_limit("host", args.step_seconds):
        m = min(n, args.host_candidates)
        off = np.asarray(table["offset"], dtype=np.int64)
        gpos = off[random_targets["contig"]] + random_targets["pos"].astype(np.int64)

        def host_once():
            t0 = time.perf_counter()
            pc, pl = C.c_void_p(), C.c_void_p()
            _lib.check(L.vsc_guides_data(h, C.byref(pc), C.byref(pl)), ctx._h)  # (the first call copies all loci out)
            t1 = time.perf_counter()
            loci = np.frombuffer((C.c_char * (m * 16)).from_address(pl.value), dtype=va.LOCUS_DTYPE)
            pos, strand = loci["pos"].astype(np.int64), loci["strand"].astype(np.int64)
            g0 = off[loci["contig"]] + np.where(strand == 1, pos + 23 - 3 - 5, pos + 3)
            first = np.searchsorted(gpos, g0)
            near = np.minimum(first, len(gpos) - 1)
            hit = (first < len(gpos)) & (gpos[near] < g0 + 5)
            return (time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3, int(hit.sum())

        runs = [host_once() for _ in range(1 + args.calls)]
        join = sorted(r[0] - r[1] for r in runs[1:])
        report("host", {"candidates_joined": m, "copy_out_all_loci_ms": runs[0][1], "join_ms": join,
                        "join_ms_scaled_to_all_candidates": join[0] * n / m, "windows_with_a_target": runs[0][2],
                        "note": "window test only: the letters are not decoded, so this is less than the device computes"})
    L.vsc_guides_free(h)
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()

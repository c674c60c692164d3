"""Prime-editing extensions of candidate guides (vsc_guides_prime, vsc_guides_filter_prime) on the synthetic hg38-sized genome of
varscot_amd.synth, one GPU, beside the enumeration that produces the candidates and the base-editor rows kernel over the same
candidates, in one run and one process (edit_bench's genome and candidates).

    python tools/prime_bench.py                      JSON to profiles/prime.json (and stdout)
    python tools/prime_bench.py --calls 1 --warmup 1 (what a kernel trace needs: run it under rocprofv3 --kernel-trace --stats)

Steps (each under its own time limit, --step-seconds: W warm-up calls, then K timed calls, fastest .. slowest)
  enumerate    vsc_guides_enumerate alone: NGG, both strands, no filter, no regions - a yardstick; kernels' time =
               vsc_timing.scan_ms (count pass + scan, write pass)
  edit_rows    + vsc_guides_edit, window (3, 5), base C, no targets: edit_rows_kernel - the other yardstick
  rows_none    + vsc_guides_prime under the PE2 preset, no edits: prime_rows_kernel = vsc_timing.score_ms
  rows_snv     the same with about 10^6 random SNVs, pairs counted only: the rows kernel, and the pairs' count pass + scan + write
               pass (coverage and pairs by flag) = vsc_timing.scan_ms; with the occupancy bitmap on and off
               (vsc_debug_prime_bitmap), in turn in the same step
  rows_exons   the same with an SNV at every fourth position of the 250 000 exon-like intervals (synth.synthetic_regions)
  groups       the rows kernel without edits and with the random SNVs under a grid of --caps workgroups per CU (28 is the
               library's default; vsc_debug_prime_groups_per_cu), the caps in turn round by round
  pairs_snv / pairs_exons   the same calls (bitmap on) with the pairs written and copied to the host
  filter       vsc_guides_filter_prime, the random SNVs, allow_weak: both passes and the scan = vsc_timing.score_ms
Reported beside each kernel time, the floors DERIVED from the shapes: 24 bytes per candidate (16 of locus read, 8
of row written) for the rows kernel, 8 bytes per candidate per pass + 16 per pair for the pairs passes, at the 6.3 TB/s a float4
copy kernel reaches."""
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
from edit_bench import targets_of_global  # noqa: E402
from efficiency_bench import FLOAT4_COPY_TBS, enumerate_once  # noqa: E402
from microhomology_bench import step_limit  # noqa: E402


def snvs_of(targets, rng):
    """PRIME_EDIT_DTYPE (strictly ascending, as the targets are): one substitution by a random letter at every target."""
    e = np.zeros(len(targets), dtype=va.PRIME_EDIT_DTYPE)
    e["contig"], e["pos"], e["del_len"], e["ins_len"] = targets["contig"], targets["pos"], 1, 1
    e["ins"] = rng.integers(0, 4, size=len(targets), dtype=np.uint32)
    return e


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--random-edits", type=int, default=1_000_000)
    ap.add_argument("--intervals", type=int, default=250_000)
    ap.add_argument("--fraction", type=float, default=0.03)
    ap.add_argument("--exon-step", type=int, default=4)
    ap.add_argument("--caps", default="7,8,14,28,56", help="the workgroups per CU of the `groups` step")
    ap.add_argument("--only-groups", action="store_true", help="the `groups` step alone (with the set-up it needs)")
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prime.json"))
    args = ap.parse_args()
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    print(json.dumps({"planes_words": int(len(hi))}), flush=True)
    rng = np.random.default_rng(30)
    random_edits = snvs_of(targets_of_global(table, np.unique(rng.integers(0, span, size=args.random_edits, dtype=np.int64))), rng)
    iv = synth.synthetic_regions(table, args.intervals, args.fraction)
    start = np.asarray(table["offset"], dtype=np.int64)[iv["contig"]] + iv["start"].astype(np.int64)
    length = (iv["end"].astype(np.int64) - iv["start"].astype(np.int64))
    g = np.repeat(start - np.concatenate(([0], np.cumsum(length)[:-1])), length) + np.arange(int(length.sum()), dtype=np.int64)
    g = np.unique(g)[::args.exon_step]
    exon_edits = snvs_of(targets_of_global(table, g), rng)
    del g
    print(json.dumps({"random_edits": len(random_edits), "exon_edits": len(exon_edits)}), flush=True)
    with step_limit("load", args.step_seconds):
        ctx = va.Context(0)
        genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    L = va.lib()
    params = _enum_params("GG", "both", (0, 0), 0, 0)
    res = {"genome_bases": args.bases, "calls": args.calls, "warmup": args.warmup, "float4_copy_tbs": FLOAT4_COPY_TBS,
           "random_edits": len(random_edits), "exon_edits": len(exon_edits), "bitmap_cell_positions": 256,
           "bitmap_bytes": (span // 256 + 8) // 8}

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

    with step_limit("edit_rows", args.step_seconds):
        cbe = va.EDITORS["CBE"]._struct()

        def edit_once():
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_edit(ctx._h, genome._h, h, C.byref(cbe), None, 0, None, None, 0, None, None, None), ctx._h)
            return (time.perf_counter() - t0) * 1e3, ctx.timing()["score_ms"]

        runs = timed(edit_once)
        report("edit_rows", {"candidates": n, "kernel_ms": sorted(r[1] for r in runs), "wall_ms": sorted(r[0] for r in runs)})
    edit_ms = res["edit_rows"]["kernel_ms"][0]

    shape = va.PRIME_EDITORS["PE2"]._struct()
    st, count = _lib.PrimeStats(), C.c_uint64()
    hbm_rows_ms = 24.0 * n / (FLOAT4_COPY_TBS * 1e12) * 1e3

    def prime_step(name, edits, write_pairs, bitmaps):
        with step_limit(name, args.step_seconds):
            n_e = 0 if edits is None else len(edits)
            pairs = None
            if write_pairs:
                _lib.check(L.vsc_guides_prime(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(edits), n_e, None, None, 0, C.byref(count), None,
                                              None), ctx._h)
                pairs = np.empty(int(count.value), dtype=va.PRIME_PAIR_DTYPE)

            def once():
                t0 = time.perf_counter()
                _lib.check(L.vsc_guides_prime(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(edits) if n_e else None, n_e, None,
                                              _lib.ptr(pairs), 0 if pairs is None else len(pairs), C.byref(count), None, C.byref(st)), ctx._h)
                wall = (time.perf_counter() - t0) * 1e3
                t = ctx.timing()
                return wall, t["score_ms"], t["scan_ms"]

            out = {"candidates": n, "edits": n_e, "rows_floor_hbm_ms": hbm_rows_ms}
            for on in bitmaps:
                _lib.check(L.vsc_debug_prime_bitmap(ctx._h, on))
                runs = timed(once)
                kernel = sorted(r[1] for r in runs)
                part = {"stats": st.as_dict(), "rows_kernel_ms": kernel, "wall_ms": sorted(r[0] for r in runs),
                        "rows_kernel_over_enumerate_kernels": kernel[0] / enum_ms, "rows_kernel_over_edit_rows_kernel": kernel[0] / edit_ms}
                if n_e:
                    # count pass: 8 B per candidate; write pass: 8 B per candidate + 16 B per pair (written only with write_pairs)
                    pass_bytes = 16.0 * n + (16.0 * st.pairs if write_pairs else 0.0)
                    part.update(pairs_passes_ms=sorted(r[2] for r in runs), pairs_written=bool(write_pairs),
                                pairs_floor_hbm_ms=pass_bytes / (FLOAT4_COPY_TBS * 1e12) * 1e3)
                out["bitmap_on" if on else "bitmap_off"] = part
            _lib.check(L.vsc_debug_prime_bitmap(ctx._h, 1))
            if len(bitmaps) == 2:  # not one output bit depends on the bitmap
                a, b = out["bitmap_on"]["stats"], out["bitmap_off"]["stats"]
                assert all(a[k] == b[k] for k in a if not k.endswith("_ms")), (a, b)
            report(name, out)

    if not args.only_groups:
        prime_step("rows_none", None, False, (1,))
        prime_step("rows_snv", random_edits, False, (1, 0))
        prime_step("rows_exons", exon_edits, False, (1, 0))
    with step_limit("groups", args.step_seconds):
        # the cap of the rows kernel's grid: its 106 SGPRs admit 7 waves per SIMD, so 7 workgroups of 4 waves per CU are resident
        # at once (8 is what edit_rows_kernel's launch starts, 28 the library's default).  The caps in turn, round by round.
        caps = tuple(int(x) for x in args.caps.split(","))

        def rows_once(edits):
            n_e = 0 if edits is None else len(edits)
            _lib.check(L.vsc_guides_prime(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(edits) if n_e else None, n_e, None, None, 0, C.byref(count),
                                          None, C.byref(st)), ctx._h)
            return ctx.timing()["score_ms"], st.pairs

        out = {}
        for key, edits in (("no_edits", None), ("random_snvs", random_edits)):
            times, pairs = {g: [] for g in caps}, set()
            for r in range(args.warmup + args.calls):
                for g in caps:
                    _lib.check(L.vsc_debug_prime_groups_per_cu(ctx._h, g))
                    ms, n_pairs = rows_once(edits)
                    pairs.add(int(n_pairs))
                    if r >= args.warmup:
                        times[g].append(ms)
            assert len(pairs) == 1, pairs
            out[key] = {"rows_kernel_ms_by_groups_per_cu": {str(g): sorted(v) for g, v in times.items()}}
        _lib.check(L.vsc_debug_prime_groups_per_cu(ctx._h, 0))
        report("groups", out)
    if args.only_groups:
        L.vsc_guides_free(h)
        genome.close()
        ctx.close()
        return

    prime_step("pairs_snv", random_edits, True, (1,))
    prime_step("pairs_exons", exon_edits, True, (1,))

    with step_limit("filter", args.step_seconds):
        def filter_once():
            out = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_filter_prime(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(random_edits), len(random_edits), 1, C.byref(out)),
                       ctx._h)
            wall = (time.perf_counter() - t0) * 1e3
            kept = int(L.vsc_guides_count(out))
            L.vsc_guides_free(out)
            t = ctx.timing()
            return wall, t["score_ms"], kept, t["genome_bytes"]

        runs = timed(filter_once)
        with_pair = res["rows_snv"]["bitmap_on"]["stats"]["with_pair"]
        assert runs[0][2] == with_pair, (runs[0][2], with_pair)
        report("filter", {"candidates": n, "edits": len(random_edits), "survivors": runs[0][2], "kernels_ms": sorted(r[1] for r in runs),
                          "wall_ms": sorted(r[0] for r in runs), "bytes": runs[0][3],
                          "floor_ms_at_float4_copy_kernel": runs[0][3] / (FLOAT4_COPY_TBS * 1e12) * 1e3})
    L.vsc_guides_free(h)
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()

"""Motif rows of candidate guides (vsc_guides_motifs, vsc_guides_filter_motifs) on the synthetic hg38-sized genome of
varscot_amd.synth, one GPU, beside the enumeration that produces the candidates, the efficiency kernel and the fold kernel
(no scaffold) over the same candidates, in one run and one process.

    python tools/motif_bench.py                      JSON to profiles/motifs.json (and stdout)
    python tools/motif_bench.py --calls 1 --warmup 1 (what a kernel trace needs: run it under rocprofv3 --kernel-trace --stats)

Steps (each under its own time limit, --step-seconds: W warm-up calls, then K timed calls, fastest .. slowest)
  enumerate      vsc_guides_enumerate alone: NGG, both strands, no filter, no regions - the yardstick; kernels' time =
                 vsc_timing.scan_ms (count pass + scan, write pass)
  efficiency     + vsc_guides_efficiency over those candidates under tools/efficiency_bench.py's model - the second yardstick
  fold_m0        + vsc_guides_fold, the SpCas9 preset, no scaffold - the third
  rows_cloning   + vsc_guides_motifs, the SpCas9 preset, BsmBI / BbsI / BsaI on both strands, flanks of 4 letters: kernel time =
                 vsc_timing.score_ms; the host wall time beside it holds the copy of 24 bytes per candidate to the host
  rows_63        the same with 63 fixed motifs of 4 .. 8 letters on both strands (the genotyping case), with the totals
  filter_cloning + vsc_guides_filter_motifs, forbid_construct on all three: both passes and the scan
Reported beside each rows kernel's time, the two floors DERIVED from the shapes:
  HBM   40 bytes per candidate (16 of locus read, 24 of row written) at the 6.3 TB/s a float4 copy kernel reaches
  VALU  the vector instructions counted in the kernel's ISA: 30 per pattern letter (16 ANDs that select the letter masks of
        both texts, 8 ORs, 2 shifts, 4 ANDs into the two match masks) and 40 per pattern (the pattern's fields out of LDS into
        scalars, the three tests and the three masked ORs into the row); 4 cycles per wave instruction and SIMD, 4 SIMDs per CU
at --clock-ghz (default 2.4, the MI355X's peak engine clock) and the device's CU count.
"""
import argparse
import contextlib
import ctypes as C
import json
import os
import signal
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
from efficiency_bench import FLOAT4_COPY_TBS, bench_model, enumerate_once  # noqa: E402

VALU_LETTER, VALU_PATTERN = 30, 40
CLONING = [("BsmBI", "CGTCTC"), ("BbsI", "GAAGAC"), ("BsaI", "GGTCTC")]
LEFT, RIGHT = "CACC", "GTTT"


def many_motifs():
    """63 fixed words of 4 .. 8 letters: the kernel's time depends on their lengths, not on their letters."""
    rng = np.random.default_rng(63)
    out = []
    while len(out) < 63:
        word = "".join("ACGT"[b] for b in rng.integers(0, 4, int(rng.integers(4, 9))))
        if word not in [w for _, w in out]:
            out.append(("m%d" % len(out), word))
    return out


def pattern_letters(entries):
    """(patterns, pattern letters) of a set on both strands: a palindrome has one pattern"""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    pats = [p for _, w in entries for p in {w, "".join(comp[c] for c in reversed(w))}]
    return len(pats), sum(len(p) for p in pats)


@contextlib.contextmanager
def step_limit(name, seconds):
    """The step's own time limit: the process ends there, with nothing more started on the device."""
    def expired(_sig, _frame):
        sys.stderr.write("step %s ran past its limit of %d s\n" % (name, seconds))
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--step-seconds", type=int, default=180)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motifs.json"))
    args = ap.parse_args()
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    with step_limit("load", args.step_seconds):
        ctx = va.Context(0)
        genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    L = va.lib()
    params = _enum_params("GG", "both", (0, 0), 0, 0)
    res = {"genome_bases": args.bases, "calls": args.calls, "warmup": args.warmup, "compute_units": cus, "clock_ghz": args.clock_ghz,
           "valu_instructions": {"pattern_letter": VALU_LETTER, "pattern": VALU_PATTERN}}

    def report(key, value):
        res[key] = value
        print(json.dumps({key: value}), flush=True)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        return [fn() for _ in range(args.calls)]

    def spread(values):  # fastest / median / slowest
        v = sorted(values)
        return [v[0], v[len(v) // 2], v[-1]]

    with step_limit("enumerate", args.step_seconds):
        runs = timed(lambda: enumerate_once(ctx, genome, params))
        n = runs[0][2]
        report("enumerate", {"candidates": n, "kernels_ms": spread(r[1] for r in runs), "wall_ms": spread(r[0] for r in runs)})
        _, _, _, h = enumerate_once(ctx, genome, params, keep=True)
    enum_ms = res["enumerate"]["kernels_ms"][0]

    with step_limit("efficiency", args.step_seconds):
        model = bench_model()
        linear = np.empty(n, dtype=np.float64)

        def eff_once():
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_efficiency(ctx._h, genome._h, h, model._h, _lib.ptr(linear), None), ctx._h)
            return (time.perf_counter() - t0) * 1e3, ctx.timing()["score_ms"]

        runs = timed(eff_once)
        report("efficiency", {"candidates": n, "kernel_ms": spread(r[1] for r in runs), "wall_ms": spread(r[0] for r in runs)})
        del linear
    eff_ms = res["efficiency"]["kernel_ms"][0]

    with step_limit("fold_m0", args.step_seconds):
        fold_shape = va.FOLD_SHAPES["SpCas9"]._struct()
        fold_rows = np.empty((n, 2), dtype=np.uint32)

        def fold_once():
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_fold(ctx._h, genome._h, h, C.byref(fold_shape), b"", 0, _lib.ptr(fold_rows), None), ctx._h)
            return (time.perf_counter() - t0) * 1e3, ctx.timing()["score_ms"]

        runs = timed(fold_once)
        report("fold_m0", {"candidates": n, "kernel_ms": spread(r[1] for r in runs), "wall_ms": spread(r[0] for r in runs)})
        del fold_rows
    fold_ms = res["fold_m0"]["kernel_ms"][0]

    shape = va.MOTIF_SHAPES["SpCas9"]._struct()
    st = _lib.MotifStats()
    rows = np.empty((n, 3), dtype=np.uint64)
    lf, rf = LEFT.encode(), RIGHT.encode()
    kept_want = None
    for key, entries, with_totals in (("rows_cloning", CLONING, False), ("rows_63", many_motifs(), True)):
        with step_limit(key, args.step_seconds):
            ms = va.motifs(entries)
            arr = ms._array()
            tot = np.zeros((len(ms), 3), dtype=np.uint64)

            def rows_once():
                t0 = time.perf_counter()
                _lib.check(L.vsc_guides_motifs(ctx._h, genome._h, h, C.byref(shape), lf, len(lf), rf, len(rf), arr, len(ms), _lib.ptr(rows),
                                               _lib.ptr(tot) if with_totals else None, C.byref(st)), ctx._h)
                wall = (time.perf_counter() - t0) * 1e3
                t = ctx.timing()
                assert t["sites"] == n and t["genome_bytes"] == 40 * n
                return wall, t["score_ms"]

            runs = timed(rows_once)
            n_pat, n_letters = pattern_letters(entries)
            valu = n_pat * VALU_PATTERN + n_letters * VALU_LETTER
            floors = {"hbm_ms": 40.0 * n / (FLOAT4_COPY_TBS * 1e12) * 1e3,
                      "valu_ms": n / 64.0 * valu * 4 / (cus * 4 * args.clock_ghz * 1e9) * 1e3}
            kernel = spread(r[1] for r in runs)
            out = {"candidates": n, "motifs": len(ms), "patterns": n_pat, "pattern_letters": n_letters, "totals": with_totals,
                   "valu_instructions_in_the_loops": valu, "stats": st.as_dict(), "kernel_ms": kernel, "wall_ms": spread(r[0] for r in runs),
                   "derived_floors_ms": floors, "kernel_over_hbm_floor": kernel[0] / floors["hbm_ms"],
                   "kernel_over_valu_floor": kernel[0] / floors["valu_ms"], "kernel_ns_per_candidate_and_pattern_letter": kernel[0] * 1e6 / n / n_letters,
                   "kernel_over_enumerate_kernels": kernel[0] / enum_ms, "kernel_over_efficiency_kernel": kernel[0] / eff_ms,
                   "kernel_over_fold_kernel_m0": kernel[0] / fold_ms}
            if with_totals:
                out["totals_sum"] = [int(v) for v in tot.sum(axis=0)]
            else:
                kept_want = int((rows[:, 0] == 0).sum())  # defined rows without a construct bit (an undefined row is all ones)
            report(key, out)
    del rows

    with step_limit("filter_cloning", args.step_seconds):
        ms = va.motifs(CLONING)
        arr = ms._array()
        limits = _lib.MotifLimits(7, 0, 0, 0)

        def filter_once():
            out = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_filter_motifs(ctx._h, genome._h, h, C.byref(shape), lf, len(lf), rf, len(rf), arr, len(ms), C.byref(limits),
                                                  C.byref(out)), ctx._h)
            wall = (time.perf_counter() - t0) * 1e3
            kept = int(L.vsc_guides_count(out))
            L.vsc_guides_free(out)
            t = ctx.timing()
            return wall, t["score_ms"], kept, t["genome_bytes"]

        runs = timed(filter_once)
        assert runs[0][2] == kept_want, (runs[0][2], kept_want)
        kernels = spread(r[1] for r in runs)
        report("filter_cloning", {"candidates": n, "forbid_construct": 7, "survivors": runs[0][2], "kernels_ms": kernels,
                                  "wall_ms": spread(r[0] for r in runs), "bytes": runs[0][3],
                                  "floor_ms_at_float4_copy_kernel": runs[0][3] / (FLOAT4_COPY_TBS * 1e12) * 1e3,
                                  "kernels_over_rows_kernel": kernels[0] / res["rows_cloning"]["kernel_ms"][0],
                                  "kernels_over_enumerate_kernels": kernels[0] / enum_ms, "kernels_over_efficiency_kernel": kernels[0] / eff_ms,
                                  "kernels_over_fold_kernel_m0": kernels[0] / fold_ms})
    L.vsc_guides_free(h)
    genome.close()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

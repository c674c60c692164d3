"""Microhomology and out-of-frame scores of candidate guides (vsc_guides_microhomology, vsc_guides_filter_microhomology) on the
synthetic hg38-sized genome of varscot_amd.synth, one GPU, beside the enumeration that produces the candidates and the
efficiency kernel over the same candidates, in one run and one process.

    python tools/microhomology_bench.py                      JSON to profiles/microhomology.json (and stdout)
    python tools/microhomology_bench.py --calls 1 --warmup 1 (what a kernel trace needs: run it under rocprofv3 --kernel-trace --stats)

Steps (each under its own time limit, --step-seconds: W warm-up calls, then K timed calls, fastest .. slowest)
  enumerate   vsc_guides_enumerate alone: NGG, both strands, no filter, no regions - the yardstick; kernels' time =
              vsc_timing.scan_ms (count pass + scan, write pass)
  efficiency  + vsc_guides_efficiency over those candidates under tools/efficiency_bench.py's model - the other yardstick
  score_f30   + vsc_guides_microhomology, site_len 23, cut 17, F = 30: kernel time = vsc_timing.score_ms; the host wall time
              beside it holds the copy of 8 bytes per candidate to the host
  score_f8    the same at F = 8
  filter      + vsc_guides_filter_microhomology at F = 30 with the median out-of-frame share (per mille, of the candidates
              whose sum is not 0) as the floor: both passes and the scan = vsc_timing.score_ms
Reported beside each score kernel's time, the two floors DERIVED from the shapes:
  HBM   24 bytes per candidate (16 of locus read, 8 of pair written) at the 6.3 TB/s a float4 copy kernel reaches
  VALU  25 vector instructions per deletion length (counted in the kernel's ISA: 2 64-bit shifts of the planes, 4 xor, 2 or, 2
        and-not with the range, 2 64-bit shifts by one, 2 or, 2 and, 2 and with the G/C plane, 4 population counts, 1 add, 2
        multiply-adds), W - 1 lengths, 4 cycles per wave instruction and SIMD, 4 SIMDs per CU
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

VALU_PER_LENGTH = 25


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
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "microhomology.json"))
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
           "valu_instructions_per_length": VALU_PER_LENGTH}

    def report(key, value):
        res[key] = value
        print(json.dumps({key: value}), flush=True)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        return [fn() for _ in range(args.calls)]

    with step_limit("enumerate", args.step_seconds):
        runs = timed(lambda: enumerate_once(ctx, genome, params))
        n = runs[0][2]
        report("enumerate", {"candidates": n, "kernels_ms": sorted(r[1] for r in runs), "wall_ms": sorted(r[0] for r in runs)})
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
        report("efficiency", {"candidates": n, "kernel_ms": sorted(r[1] for r in runs), "wall_ms": sorted(r[0] for r in runs)})
        del linear

    pairs = np.empty((n, 2), dtype=np.uint32)
    st = _lib.MhStats()
    for flank in (30, 8):
        with step_limit("score_f%d" % flank, args.step_seconds):
            shape = _lib.MhShape(23, 17, flank, 0)

            def score_once():
                t0 = time.perf_counter()
                _lib.check(L.vsc_guides_microhomology(ctx._h, genome._h, h, C.byref(shape), _lib.ptr(pairs), C.byref(st)), ctx._h)
                wall = (time.perf_counter() - t0) * 1e3
                t = ctx.timing()
                assert t["sites"] == n and t["genome_bytes"] == 24 * n
                return wall, t["score_ms"]

            runs = timed(score_once)
            lengths = 2 * flank - 1
            floors = {"hbm_ms": 24.0 * n / (FLOAT4_COPY_TBS * 1e12) * 1e3,
                      "valu_ms": n / 64.0 * lengths * VALU_PER_LENGTH * 4 / (cus * 4 * args.clock_ghz * 1e9) * 1e3}
            kernel = sorted(r[1] for r in runs)
            report("score_f%d" % flank, {"candidates": n, "flank": flank, "stats": st.as_dict(), "kernel_ms": kernel,
                                         "wall_ms": sorted(r[0] for r in runs), "derived_floors_ms": floors,
                                         "kernel_over_enumerate_kernels": kernel[0] / enum_ms,
                                         "kernel_over_efficiency_kernel": kernel[0] / res["efficiency"]["kernel_ms"][0]})
        if flank == 30:
            scored = pairs[(pairs[:, 0] != va.MH_UNDEFINED) & (pairs[:, 0] > 0)]
            share = (1000 * scored[:, 1].astype(np.uint64)) // scored[:, 0].astype(np.uint64)
            permille = int(np.median(share))
            want = int(((pairs[:, 0] != va.MH_UNDEFINED) & (pairs[:, 0] > 0) &
                        (1000 * pairs[:, 1].astype(np.uint64) >= permille * pairs[:, 0].astype(np.uint64))).sum())
            del scored, share

    with step_limit("filter", args.step_seconds):
        shape = _lib.MhShape(23, 17, 30, 0)

        def filter_once():
            out = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_filter_microhomology(ctx._h, genome._h, h, C.byref(shape), 0, permille, C.byref(out)), ctx._h)
            wall = (time.perf_counter() - t0) * 1e3
            kept = int(L.vsc_guides_count(out))
            L.vsc_guides_free(out)
            t = ctx.timing()
            return wall, t["score_ms"], kept, t["genome_bytes"]

        runs = timed(filter_once)
        assert runs[0][2] == want, (runs[0][2], want)
        report("filter", {"candidates": n, "flank": 30, "min_oof_permille": permille, "survivors": runs[0][2],
                          "kernels_ms": sorted(r[1] for r in runs), "wall_ms": sorted(r[0] for r in runs), "bytes": runs[0][3],
                          "floor_ms_at_float4_copy_kernel": runs[0][3] / (FLOAT4_COPY_TBS * 1e12) * 1e3})
    L.vsc_guides_free(h)
    genome.close()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

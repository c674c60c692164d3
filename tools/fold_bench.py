"""Self-complementarity rows of candidate guides (vsc_guides_fold, vsc_guides_filter_fold) on the synthetic hg38-sized genome of
varscot_amd.synth, one GPU, beside the enumeration that produces the candidates, the efficiency kernel and the microhomology
kernel (F = 30) over the same candidates, in one run and one process.

    python tools/fold_bench.py                      JSON to profiles/fold.json (and stdout)
    python tools/fold_bench.py --calls 1 --warmup 1 (what a kernel trace needs: run it under rocprofv3 --kernel-trace --stats)

Steps (each under its own time limit, --step-seconds: W warm-up calls, then K timed calls, fastest .. slowest)
  enumerate      vsc_guides_enumerate alone: NGG, both strands, no filter, no regions - the yardstick; kernels' time =
                 vsc_timing.scan_ms (count pass + scan, write pass)
  efficiency     + vsc_guides_efficiency over those candidates under tools/efficiency_bench.py's model - the second yardstick
  microhomology  + vsc_guides_microhomology at F = 30 - the third
  rows_m0        + vsc_guides_fold, the SpCas9 preset, no scaffold: kernel time = vsc_timing.score_ms; the host wall time beside
                 it holds the copy of 8 bytes per candidate to the host
  rows_m20, rows_m76   the same against a fixed scaffold text of 20 and of 76 letters
  filter         + vsc_guides_filter_fold at m = 76 with the median starts as max_starts: both passes and the scan
Reported beside each rows kernel's time, the two floors DERIVED from the shapes:
  HBM   24 bytes per candidate (16 of locus read, 8 of row written) at the 6.3 TB/s a float4 copy kernel reaches
  VALU  per diagonal the vector instructions counted in the kernel's ISA - 23 on a diagonal of the spacer against itself (2
        shifts of the reversal, 3 for the pairs, the compare in front of the run search and the move into it, 5 for the k-run
        starts and QUAL, 3 for the cover, 1 shift of the 3' cover, 3 to keep starts, cover and 3' cover, the move and the
        maximum of the longest run, 2 moves), 16 on a diagonal against the scaffold (the address move, 4 for the pairs and the
        window's mask, the compare, 9 for starts, QUAL, cover and keeping them, the maximum) - and 4 per turn of the longest-run
        search, of which every diagonal takes at least one; 2 n - 2 - min_loop and n + m - 1 diagonals; 4 cycles per wave
        instruction and SIMD, 4 SIMDs per CU
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

VALU_SELF, VALU_SCAFFOLD, VALU_RUN_TURN = 23, 16, 4
# any fixed text will do: the kernel's time does not depend on the letters
SCAFFOLD = "GUUUUAGAGCUAGAAAUAGCAAGUUAAAAUAAGGCUAGUCCGUUAUCAACUUGAAAAAGUGGCACCGAGUCGGUGC"


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold.json"))
    args = ap.parse_args()
    assert len(SCAFFOLD) == 76
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
           "valu_instructions": {"self_diagonal": VALU_SELF, "scaffold_diagonal": VALU_SCAFFOLD, "run_search_turn": VALU_RUN_TURN}}

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

    rows = np.empty((n, 2), dtype=np.uint32)
    with step_limit("microhomology", args.step_seconds):
        mh_shape = _lib.MhShape(23, 17, 30, 0)

        def mh_once():
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_microhomology(ctx._h, genome._h, h, C.byref(mh_shape), _lib.ptr(rows), None), ctx._h)
            return (time.perf_counter() - t0) * 1e3, ctx.timing()["score_ms"]

        runs = timed(mh_once)
        report("microhomology", {"candidates": n, "flank": 30, "kernel_ms": spread(r[1] for r in runs), "wall_ms": spread(r[0] for r in runs)})
    mh_ms = res["microhomology"]["kernel_ms"][0]

    preset = va.FOLD_SHAPES["SpCas9"]
    shape = preset._struct()
    st = _lib.FoldStats()
    for m in (0, 20, 76):
        with step_limit("rows_m%d" % m, args.step_seconds):
            sc = SCAFFOLD[:m].encode()

            def rows_once():
                t0 = time.perf_counter()
                _lib.check(L.vsc_guides_fold(ctx._h, genome._h, h, C.byref(shape), sc, m, _lib.ptr(rows), C.byref(st)), ctx._h)
                wall = (time.perf_counter() - t0) * 1e3
                t = ctx.timing()
                assert t["sites"] == n and t["genome_bytes"] == 24 * n
                return wall, t["score_ms"]

            runs = timed(rows_once)
            self_diagonals = 2 * preset.proto_len - 2 - preset.min_loop
            scaf_diagonals = preset.proto_len + m - 1 if m else 0
            valu = self_diagonals * (VALU_SELF + VALU_RUN_TURN) + scaf_diagonals * (VALU_SCAFFOLD + VALU_RUN_TURN)
            floors = {"hbm_ms": 24.0 * n / (FLOAT4_COPY_TBS * 1e12) * 1e3,
                      "valu_ms": n / 64.0 * valu * 4 / (cus * 4 * args.clock_ghz * 1e9) * 1e3}
            kernel = spread(r[1] for r in runs)
            u = va.unpack_fold_row(rows[:: max(1, n // 1_000_000)])
            report("rows_m%d" % m, {"candidates": n, "scaffold_letters": m, "self_diagonals": self_diagonals, "scaffold_diagonals": scaf_diagonals,
                                    "valu_instructions_in_the_loops": valu, "stats": st.as_dict(), "kernel_ms": kernel,
                                    "wall_ms": spread(r[0] for r in runs), "derived_floors_ms": floors,
                                    "kernel_over_valu_floor": kernel[0] / floors["valu_ms"],
                                    "kernel_over_enumerate_kernels": kernel[0] / enum_ms, "kernel_over_efficiency_kernel": kernel[0] / eff_ms,
                                    "kernel_over_microhomology_kernel": kernel[0] / mh_ms,
                                    "sampled_means": {k: float(v[u["defined"]].mean()) for k, v in u.items() if k != "defined"}})
    u = va.unpack_fold_row(rows)
    max_starts = int(np.median(u["starts"][u["defined"]]))
    want = int((u["defined"] & (u["starts"] <= max_starts)).sum())
    del u

    with step_limit("filter", args.step_seconds):
        sc = SCAFFOLD.encode()
        limits = _lib.FoldLimits(max_starts, va.FOLD_NO_LIMIT, va.FOLD_NO_LIMIT, va.FOLD_NO_LIMIT)

        def filter_once():
            out = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.vsc_guides_filter_fold(ctx._h, genome._h, h, C.byref(shape), sc, len(sc), C.byref(limits), C.byref(out)), ctx._h)
            wall = (time.perf_counter() - t0) * 1e3
            kept = int(L.vsc_guides_count(out))
            L.vsc_guides_free(out)
            t = ctx.timing()
            return wall, t["score_ms"], kept, t["genome_bytes"]

        runs = timed(filter_once)
        assert runs[0][2] == want, (runs[0][2], want)
        kernels = spread(r[1] for r in runs)
        report("filter", {"candidates": n, "scaffold_letters": 76, "max_starts": max_starts, "survivors": runs[0][2], "kernels_ms": kernels,
                          "wall_ms": spread(r[0] for r in runs), "bytes": runs[0][3],
                          "floor_ms_at_float4_copy_kernel": runs[0][3] / (FLOAT4_COPY_TBS * 1e12) * 1e3,
                          "kernels_over_rows_kernel_m76": kernels[0] / res["rows_m76"]["kernel_ms"][0],
                          "kernels_over_enumerate_kernels": kernels[0] / enum_ms, "kernels_over_efficiency_kernel": kernels[0] / eff_ms,
                          "kernels_over_microhomology_kernel": kernels[0] / mh_ms})
    L.vsc_guides_free(h)
    genome.close()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

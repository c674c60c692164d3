"""On-target efficiency of candidate guides (vsc_guides_efficiency, vsc_guides_filter_efficiency) on the synthetic hg38-sized
genome of varscot_amd.synth, one GPU, beside the enumeration that produces the candidates, in one run.

    python tools/efficiency_bench.py                      JSON to profiles/efficiency.json (and stdout)
    python tools/efficiency_bench.py --calls 1 --warmup 1 (what a kernel trace needs: run it under rocprofv3 --kernel-trace --stats)

Steps (each: W warm-up calls, then K timed calls, fastest .. slowest)
  enumerate   vsc_guides_enumerate alone: NGG, both strands, no filter, no regions - the yardstick (tools/enumerate_bench.py's
              genome case); kernels' time = vsc_timing.scan_ms (count pass + scan, write pass)
  score       + vsc_guides_efficiency over those candidates where they lie on the device, under a dense model of the Rule Set 1
              shape (4 + 23 + 3 bases, C = 30, a G/C table over the 20 protospacer bases): kernel time = vsc_timing.score_ms;
              the host wall time beside it holds the copy of 8 bytes per candidate to the host
  filter      + vsc_guides_filter_efficiency with the median predictor as the floor: both passes and the scan =
              vsc_timing.score_ms; the result stays on the device and is freed again
Reported beside the score kernel's time, the three floors DERIVED from the shapes:
  HBM   24 bytes per candidate (16 of locus read, 8 of score written) at the 6.3 TB/s a float4 copy kernel reaches
  LDS   2 C - 1 ds_read_b64 per candidate, 64 candidates per wave instruction, 2 LDS cycles per wave instruction and CU
  VALU  5 vector instructions per term, 4 cycles per wave instruction and SIMD, 4 SIMDs per CU
at --clock-ghz (default 2.4, the MI355X's peak engine clock) and the device's CU count.
"""
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

import varscot_amd as va  # noqa: E402
from varscot_amd import _lib, dist as vdist, synth  # noqa: E402
from varscot_amd.api import _enum_params  # noqa: E402

FLOAT4_COPY_TBS = 6.3  # DESIGN 8 item 3 (tools/gpu.sh bw)
SHAPE = (4, 23, 3)


def bench_model():
    rng = np.random.default_rng(2014)
    c = sum(SHAPE)
    return va.EfficiencyModel(SHAPE[0], SHAPE[1], SHAPE[2], 0.6, rng.normal(scale=0.1, size=(c, 4)), rng.normal(scale=0.1, size=(c - 1, 16)),
                              gc=rng.normal(scale=0.1, size=21), gc_range=(SHAPE[0], 20))


def enumerate_once(ctx, genome, params, keep=False):
    """(wall ms, kernels ms, candidates[, handle]) of one vsc_guides_enumerate"""
    L = va.lib()
    h = C.c_void_p()
    t0 = time.perf_counter()
    _lib.check(L.vsc_guides_enumerate(ctx._h, genome._h, None, C.byref(params), C.byref(h)), ctx._h)
    wall = (time.perf_counter() - t0) * 1e3
    n = int(L.vsc_guides_count(h))
    ms = ctx.timing()["scan_ms"]
    if keep:
        return wall, ms, n, h
    L.vsc_guides_free(h)
    return wall, ms, n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "efficiency.json"))
    args = ap.parse_args()
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    L = va.lib()
    model = bench_model()
    params = _enum_params("GG", "both", (0, 0), 0, 0)
    res = {"genome_bases": args.bases, "calls": args.calls, "warmup": args.warmup, "compute_units": cus, "clock_ghz": args.clock_ghz,
           "model": {"shape": list(SHAPE), "context": sum(SHAPE), "gc_range": [SHAPE[0], 20], "weights": "dense, seeded"}}

    def report(key, value):
        res[key] = value
        print(json.dumps({key: value}), flush=True)

    for _ in range(args.warmup):
        enumerate_once(ctx, genome, params)
    runs = [enumerate_once(ctx, genome, params) for _ in range(args.calls)]
    n = runs[0][2]
    report("enumerate", {"candidates": n, "kernels_ms": sorted(r[1] for r in runs), "wall_ms": sorted(r[0] for r in runs)})

    _, _, _, h = enumerate_once(ctx, genome, params, keep=True)
    linear = np.empty(n, dtype=np.float64)
    st = _lib.EffStats()

    def score_once():
        t0 = time.perf_counter()
        _lib.check(L.vsc_guides_efficiency(ctx._h, genome._h, h, model._h, _lib.ptr(linear), C.byref(st)), ctx._h)
        wall = (time.perf_counter() - t0) * 1e3
        t = ctx.timing()
        assert t["sites"] == n and t["genome_bytes"] == 24 * n
        return wall, t["score_ms"]

    for _ in range(args.warmup):
        score_once()
    runs = [score_once() for _ in range(args.calls)]
    terms = 2 * sum(SHAPE) - 1
    waves = n / 64.0
    floors = {"hbm_ms": 24.0 * n / (FLOAT4_COPY_TBS * 1e12) * 1e3,
              "lds_ms": waves * terms * 2 / (cus * args.clock_ghz * 1e9) * 1e3,
              "valu_ms": waves * terms * 5 * 4 / (cus * 4 * args.clock_ghz * 1e9) * 1e3}
    kernel = sorted(r[1] for r in runs)
    report("score", {"candidates": n, "stats": st.as_dict(), "kernel_ms": kernel, "wall_ms": sorted(r[0] for r in runs),
                     "derived_floors_ms": floors, "kernel_over_enumerate_kernels": kernel[0] / res["enumerate"]["kernels_ms"][0],
                     "bytes_per_s_at_fastest": 24.0 * n / (kernel[0] * 1e-3) if kernel[0] > 0 else None})

    defined = ~np.isnan(linear)
    floor = float(np.median(linear[defined]))

    def filter_once():
        out = C.c_void_p()
        t0 = time.perf_counter()
        _lib.check(L.vsc_guides_filter_efficiency(ctx._h, genome._h, h, model._h, floor, C.byref(out)), ctx._h)
        wall = (time.perf_counter() - t0) * 1e3
        kept = int(L.vsc_guides_count(out))
        L.vsc_guides_free(out)
        t = ctx.timing()
        return wall, t["score_ms"], kept, t["genome_bytes"]

    for _ in range(args.warmup):
        filter_once()
    runs = [filter_once() for _ in range(args.calls)]
    assert runs[0][2] == int((linear[defined] >= floor).sum())
    report("filter", {"candidates": n, "floor": floor, "survivors": runs[0][2], "kernels_ms": sorted(r[1] for r in runs),
                      "wall_ms": sorted(r[0] for r in runs), "bytes": runs[0][3],
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

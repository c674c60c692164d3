"""The per-target pick (vsc_guides_pick) on the synthetic hg38-sized genome of varscot_amd.synth, one GPU, one
process.

    python tools/pick_bench.py                 all steps, JSON to profiles/pick.json (and stdout, step by step)
    python tools/pick_bench.py --calls 1 --warmup 1 --steps exons     (what a kernel trace needs)

The candidates are those of the 250 000-interval exon-like annotation of tools/enumerate_bench.py (overlap rule, NGG, both
strands); they stay on the device.  The keys are 14-bit integers (what rint(100 x specificity) gives), drawn once.  Steps, each
under its own time limit (SIGALRM ends the process; what was measured before is already in the JSON file), each W warm-up
calls and then K timed calls:
  enumerate  vsc_guides_enumerate of the same targets: the kernels' time (vsc_timing.scan_ms), for comparison
  exons      one target per interval, labels made on the device, K = 4, spacing 20
  genes      the same intervals grouped 8 per gene (group[]), K = 4, spacing 20
  one        every candidate in ONE target (a target array of zeros), K = 32, spacing 20: the worst case - one wave walks
             the whole segment once per round
  host       vsc_pick_host on the copied-out arrays: the copy of the loci, vsc_guides_locate for the labels and the host pick
Per device step: the stages' times (mark + scan, scatter, select, rank: vsc_pick_stats.stage_ms), the call's wall time, the
counts, a derived HBM floor at 6.3 TB/s - mark: 16 + 8 bytes read and 4 written per candidate; scatter: 16 + 8 + 4 read per
candidate and 20 written per eligible record; select: 20 read per eligible record, 4 k + 4 written per target - and a derived
issue estimate for the select: rounds x (records per lane + exchange steps) wave instructions per target.
"""
import argparse
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

import varscot_amd as va  # noqa: E402
from varscot_amd import _lib, dist as vdist, synth  # noqa: E402
from varscot_amd.api import _enum_params  # noqa: E402

HBM_TBS = 6.3
PER_LANE = 4          # kPickPerLane
EXCHANGE = 6 * 3 + 3  # wave_first: six butterfly steps of three words; the ballot and the two broadcasts of the winner


def pick_call(ctx, genome, h, n, key, n_targets, shape, regions=None, group=None, target=None):
    L = va.lib()
    picks = np.empty((n_targets, shape.k), dtype=np.uint32)
    counts = np.empty(n_targets, dtype=np.uint32)
    st = _lib.PickStats()
    sh = shape._struct()
    t0 = time.perf_counter()
    _lib.check(L.vsc_guides_pick(ctx._h, genome._h, h, regions._h if regions is not None else None, _lib.ptr(group) if group is not None else None,
                                 _lib.ptr(target) if target is not None else None, n_targets, _lib.ptr(key), C.byref(sh), _lib.ptr(picks),
                                 _lib.ptr(counts), None, None, C.byref(st)), ctx._h)
    wall = (time.perf_counter() - t0) * 1e3
    return wall, st.as_dict(), picks, counts


def device_step(ctx, genome, h, n, key, n_targets, shape, calls, warmup, **kw):
    for _ in range(warmup):
        pick_call(ctx, genome, h, n, key, n_targets, shape, **kw)
    runs = [pick_call(ctx, genome, h, n, key, n_targets, shape, **kw) for _ in range(calls)]
    st = runs[0][1]
    assert all(r[2].tobytes() == runs[0][2].tobytes() and r[3].tobytes() == runs[0][3].tobytes() for r in runs)
    e = st["eligible"]
    floor = {"mark": 28 * n, "scatter": 28 * n + 20 * e, "select": 20 * e + (4 * shape.k + 4) * n_targets}
    largest = int(np.bincount(np.minimum(runs[0][3], shape.k)).argmax())
    return {"candidates": n, "targets": n_targets, "k": shape.k, "spacing": shape.spacing,
            "counts": {k: v for k, v in st.items() if not k.endswith("_ms")},
            "stage_ms": {name: sorted(r[1]["stage_ms"][i] for r in runs) for i, name in enumerate(("mark_scan", "scatter", "select", "rank"))},
            "kernel_ms": sorted(r[1]["kernel_ms"] for r in runs), "wall_ms": sorted(r[0] for r in runs),
            "floor_bytes": floor, "floor_ms_at_6.3_tb_per_s": {k: v / (HBM_TBS * 1e12) * 1e3 for k, v in floor.items()},
            "select_issue_estimate_per_target": shape.k * (PER_LANE + EXCHANGE), "most_common_count": largest}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=int, default=3_000_000_000)
    ap.add_argument("--intervals", type=int, default=250_000)
    ap.add_argument("--fraction", type=float, default=0.03)
    ap.add_argument("--steps", default="enumerate,exons,genes,one,host")
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pick.json"))
    args = ap.parse_args()
    steps = args.steps.split(",")
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    iv = synth.synthetic_regions(table, args.intervals, args.fraction)
    regions = va.Regions(va.PackedGenome(None, None, None, table), iv, rule="overlap")
    res = {"genome_bases": args.bases, "intervals": args.intervals, "fraction": args.fraction, "calls": args.calls, "warmup": args.warmup,
           "hbm_tb_per_s": HBM_TBS, "steps": {}}

    def report(name, value):
        res["steps"][name] = value
        print(json.dumps({name: value}), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    L = va.lib()
    plain = _enum_params("GG", "both", (0, 0), 0, 0)
    h = C.c_void_p()
    enum_ms = []
    for i in range(args.warmup + args.calls):
        signal.alarm(args.limit)
        if h:
            L.vsc_guides_free(h)
            h = C.c_void_p()
        _lib.check(L.vsc_guides_enumerate(ctx._h, genome._h, regions._h, C.byref(plain), C.byref(h)), ctx._h)
        if i >= args.warmup:
            enum_ms.append(ctx.timing()["scan_ms"])
        signal.alarm(0)
    n = int(L.vsc_guides_count(h))
    if "enumerate" in steps:
        report("enumerate", {"candidates": n, "kernels_ms": sorted(enum_ms)})
    key = np.random.default_rng(1).integers(0, 10001, n).astype(np.uint64)
    shape = va.PickShape(4, 20)
    if "exons" in steps:
        signal.alarm(args.limit)
        report("exons", device_step(ctx, genome, h, n, key, args.intervals, shape, args.calls, args.warmup, regions=regions))
        signal.alarm(0)
    if "genes" in steps:
        signal.alarm(args.limit)
        group = (np.arange(args.intervals) // 8).astype(np.uint32)
        report("genes", device_step(ctx, genome, h, n, key, int(group.max()) + 1, shape, args.calls, args.warmup, regions=regions, group=group))
        signal.alarm(0)
    if "one" in steps:
        signal.alarm(args.limit)
        report("one", device_step(ctx, genome, h, n, key, 1, va.PickShape(32, 20), args.calls, args.warmup, target=np.zeros(n, dtype=np.uint32)))
        signal.alarm(0)
    if "host" in steps:
        signal.alarm(args.limit)
        t0 = time.perf_counter()
        pc, pl = C.c_void_p(), C.c_void_p()
        _lib.check(L.vsc_guides_data(h, C.byref(pc), C.byref(pl)), ctx._h)
        loci = np.frombuffer((C.c_char * (n * 16)).from_address(pl.value), dtype=va.LOCUS_DTYPE)
        t_copy = time.perf_counter()
        labels = np.empty(n, dtype=np.uint32)
        _lib.check(L.vsc_guides_locate(h, regions._h, _lib.ptr(labels)), ctx._h)
        t_locate = time.perf_counter()
        got = va.pick_host(table, loci, labels, key, args.intervals, shape)
        t_pick = time.perf_counter()
        report("host", {"copy_ms": (t_copy - t0) * 1e3, "locate_ms": (t_locate - t_copy) * 1e3, "pick_host_ms": (t_pick - t_locate) * 1e3,
                        "total_ms": (t_pick - t0) * 1e3, "counts": {k: v for k, v in got[2].items() if not k.endswith("_ms")}})
        if "exons" in res["steps"]:
            assert res["steps"]["exons"]["counts"] == res["steps"]["host"]["counts"]
        signal.alarm(0)
    L.vsc_guides_free(h)
    regions.close()
    genome.close()
    ctx.close()


if __name__ == "__main__":
    main()

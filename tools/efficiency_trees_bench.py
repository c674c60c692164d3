"""On-target efficiency from regression-tree ensembles (vsc_guides_efficiency_trees, vsc_guides_filter_efficiency_trees) on the
synthetic hg38-sized genome of varscot_amd.synth, one GPU, beside the enumeration that produces the candidates and the linear
model's kernel, in one run - tools/efficiency_bench.py's genome and candidates.

    python tools/efficiency_trees_bench.py                      JSON to profiles/efficiency_trees.json (and stdout)
    python tools/efficiency_trees_bench.py --calls 1 --warmup 1 (what a kernel trace needs: run it under rocprofv3 --kernel-trace --stats)

Steps (each: W warm-up calls, then K timed calls, fastest .. slowest)
  enumerate     vsc_guides_enumerate alone: NGG, both strands, no filter, no regions; kernels' time = vsc_timing.scan_ms
  linear        vsc_guides_efficiency under efficiency_bench's dense model (4 + 23 + 3 bases, C = 30): the yardstick kernel
  trees_100x3   vsc_guides_efficiency_trees, 100 complete trees of depth 3, the four node kinds mixed, 3 sums (the G/C count
                of the protospacer, a letter's count over the context, a dinucleotide-weighted sum): the size of Rule Set 2
  trees_512x3   ... 512 such trees
  trees_8192    ... the largest model: 544 trees of depth 3, one of depth 4, one leaf - 8 192 nodes - and 16 sums
  filter        vsc_guides_filter_efficiency_trees under trees_100x3 with the median predictor as the floor
Every tree step reports its kernel time (vsc_timing.score_ms) beside three floors DERIVED from the model:
  HBM   24 bytes per candidate (16 of locus read, 8 of score written) at the 6.3 TB/s a float4 copy kernel reaches
  LDS   one ds_read_b64 per node visited (a complete tree of depth d: d + 1, the leaf included), 64 candidates per wave
        instruction, 2 LDS cycles per wave instruction and CU
  VALU  --valu-per-visit vector instructions per node visited (default 22: what the walk's loop body holds, the node kinds in equal parts), 4 cycles per
        wave instruction and SIMD, 4 SIMDs per CU
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
LETTERS = "ACGT"
DINUCS = [x + y for x in LETTERS for y in LETTERS]


def linear_model():
    """tools/efficiency_bench.py's model"""
    rng = np.random.default_rng(2014)
    c = sum(SHAPE)
    return va.EfficiencyModel(SHAPE[0], SHAPE[1], SHAPE[2], 0.6, rng.normal(scale=0.1, size=(c, 4)), rng.normal(scale=0.1, size=(c - 1, 16)),
                              gc=rng.normal(scale=0.1, size=21), gc_range=(SHAPE[0], 20))


def complete_tree(rng, depth, sums, typical):
    """A complete tree of `depth` numbered level by level; typical[i]: a value S_i takes, for the thresholds."""
    c = sum(SHAPE)
    inner = 2 ** depth - 1
    nodes = []
    for k in range(2 * inner + 1):
        if k >= inner:
            nodes.append(("leaf", float(rng.normal(scale=0.05))))
            continue
        kind = int(rng.integers(3 if sums else 2))
        if kind == 0:
            test = ("base", int(rng.integers(c)), "".join(ch for ch in LETTERS if rng.random() < 0.5))
        elif kind == 1:
            a = int(rng.integers(c - 1))
            test = ("pair", a, a + 1, [d for d in DINUCS if rng.random() < 0.3])
        else:
            i = int(rng.integers(len(sums)))
            test = ("sum", i, int(typical[i] + rng.integers(-2, 3)))
        nodes.append(test + (2 * k + 1, 2 * k + 2))
    return nodes


def tree_model(n_trees, seed, largest=False):
    rng = np.random.default_rng(seed)
    c = sum(SHAPE)
    sums = [(SHAPE[0], 20, {"G": 1, "C": 1}), (0, c, {"T": 1}), (SHAPE[0], 23, {d: int(w) for d, w in zip(DINUCS, rng.integers(-300, 100, 16))})]
    typical = [10, c // 4, -100 * 22]
    if largest:
        for _ in range(13):
            start = int(rng.integers(0, c - 8))
            sums.append((start, int(rng.integers(4, c - start + 1)), {LETTERS[int(rng.integers(4))]: 1, DINUCS[int(rng.integers(16))]: 3}))
            typical.append(sums[-1][1] // 4)
    trees = [complete_tree(rng, 3, sums, typical) for _ in range(n_trees)]
    if largest:
        trees += [complete_tree(rng, 4, sums, typical), [("leaf", 0.01)]]
    visits = sum((len(t) + 1).bit_length() - 1 for t in trees)  # a complete tree of depth d has 2^(d+1) - 1 nodes: d + 1 visits
    return va.TreeEfficiencyModel(SHAPE[0], SHAPE[1], SHAPE[2], 0.5, sums, trees), visits


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
    ap.add_argument("--valu-per-visit", type=float, default=22.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "efficiency_trees.json"))
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
    params = _enum_params("GG", "both", (0, 0), 0, 0)
    res = {"genome_bases": args.bases, "calls": args.calls, "warmup": args.warmup, "compute_units": cus, "clock_ghz": args.clock_ghz,
           "valu_per_visit": args.valu_per_visit, "shape": list(SHAPE)}

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

    def score_step(fn, model):
        def once():
            t0 = time.perf_counter()
            _lib.check(fn(ctx._h, genome._h, h, model._h, _lib.ptr(linear), C.byref(st)), ctx._h)
            wall = (time.perf_counter() - t0) * 1e3
            t = ctx.timing()
            assert t["sites"] == n and t["genome_bytes"] == 24 * n
            return wall, t["score_ms"]

        for _ in range(args.warmup):
            once()
        runs = [once() for _ in range(args.calls)]
        return {"kernel_ms": sorted(r[1] for r in runs), "wall_ms": sorted(r[0] for r in runs), "stats": st.as_dict()}

    lin = score_step(L.vsc_guides_efficiency, linear_model())
    lin["kernel_over_enumerate_kernels"] = lin["kernel_ms"][0] / res["enumerate"]["kernels_ms"][0]
    report("linear", lin)

    waves = n / 64.0
    models = {"trees_100x3": tree_model(100, 2016), "trees_512x3": tree_model(512, 2017), "trees_8192": tree_model(544, 2018, largest=True)}
    for key, (model, visits) in models.items():
        step = score_step(L.vsc_guides_efficiency_trees, model)
        info = model.info()
        fastest = step["kernel_ms"][0]
        step.update({"model": {k: info[k] for k in ("n_sums", "n_trees", "n_nodes", "leaves", "base_nodes", "pair_nodes", "sum_nodes", "max_depth")},
                     "node_visits_per_candidate": visits, "node_visits": visits * n,
                     "node_visits_per_s_at_fastest": visits * n / (fastest * 1e-3) if fastest > 0 else None,
                     "derived_floors_ms": {"hbm_ms": 24.0 * n / (FLOAT4_COPY_TBS * 1e12) * 1e3,
                                           "lds_ms": waves * visits * 2 / (cus * args.clock_ghz * 1e9) * 1e3,
                                           "valu_ms": waves * visits * args.valu_per_visit * 4 / (cus * 4 * args.clock_ghz * 1e9) * 1e3},
                     "kernel_over_linear_kernel": fastest / lin["kernel_ms"][0],
                     "kernel_over_enumerate_kernels": fastest / res["enumerate"]["kernels_ms"][0]})
        report(key, step)
        if key == "trees_100x3":
            defined = ~np.isnan(linear)
            floor = float(np.median(linear[defined]))
            want_kept = int((linear[defined] >= floor).sum())

    model = models["trees_100x3"][0]

    def filter_once():
        out = C.c_void_p()
        t0 = time.perf_counter()
        _lib.check(L.vsc_guides_filter_efficiency_trees(ctx._h, genome._h, h, model._h, floor, C.byref(out)), ctx._h)
        wall = (time.perf_counter() - t0) * 1e3
        kept = int(L.vsc_guides_count(out))
        L.vsc_guides_free(out)
        t = ctx.timing()
        return wall, t["score_ms"], kept, t["genome_bytes"]

    for _ in range(args.warmup):
        filter_once()
    runs = [filter_once() for _ in range(args.calls)]
    assert runs[0][2] == want_kept
    report("filter", {"candidates": n, "model": "trees_100x3", "floor": floor, "survivors": runs[0][2], "kernels_ms": sorted(r[1] for r in runs),
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

"""Guide discovery (vsc_guides_enumerate) on the synthetic hg38-sized genome of varscot_amd.synth, one GPU.

    python tools/enumerate_bench.py                       both cases, JSON to profiles/enumerate.json (and stdout)
    python tools/enumerate_bench.py --case regions --calls 1 --warmup 1     (what a kernel trace needs)
    python tools/enumerate_bench.py --locate              the labelling of the exon-like candidates, JSON to profiles/locate.json
    python tools/enumerate_bench.py --pattern             pattern guide discovery (vsc_guides_enumerate_pattern), JSON to
                                                          profiles/pattern_enum.json; --pattern-case NAME: that case alone

Cases
  genome   every candidate of the whole genome: NGG, both strands, no filter, no regions
  regions  the candidates of the 250 000-interval exon-like annotation (synth.synthetic_regions, 3 % of the genome), under both
           rules (+ the same with CRISPOR-like filters: GC 8..14 of 20, no TTTT)
Every case: W warm-up calls, then K timed calls, fastest .. slowest.  A call is the C entry point alone - the result stays on
the device and is freed again (the host copy of 4e8 candidates would time the PCIe link): host wall time per call (it contains
the hipMalloc of the result, which the context cannot pool: the caller owns it) and the enumeration kernels' own time
(vsc_timing.scan_ms: count pass + scan, write pass).
Reported beside them: candidates, the BYTE FLOOR from the shapes - plane bytes read per pass (vsc_timing.genome_bytes: 768
bytes per visited tile and pass) + 24 bytes written per candidate - and floor / kernel time against the copy bandwidths DESIGN
8 item 3 records for this part (library device-to-device copy 4.56 TB/s, float4 copy kernel 6.3 TB/s).
--locate: the candidates of the exon-like annotation (overlap, no filter) stay on the device and vsc_guides_locate labels them
against the same annotation: the first call (it uploads the label structure: 12 bytes per interval), then W warm-up and K timed
calls - host wall time per call, which holds the kernel and the copy of 4 bytes per candidate to the host; the library's own
laps (upload / kernel / copy, vsc_debug_set_host_timing) go to stderr beside it.  Floor: 16 bytes read + 4 written per record.
--pattern: the same measurement of vsc_guides_enumerate_pattern, case by case:
  spcas9        N x 21 + GG, protospacer (0, 20) - beside vsc_guides_enumerate (pam GG) in the same run, which produces the same
                candidates and the same 24 bytes per candidate; the ratio of the two kernel times is reported
  sacas9        N x 21 + NNGRRT, protospacer (0, 21)
  cas12a        TTTV + N x 23, protospacer (4, 23)
  spcas9_gc_t   spcas9 with GC 8..14 and no TTTT
  exons         spcas9 in the exon-like target set (both rules): the intervals go in as they are, the tiles that meet one are visited
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

COPY_TBS = {"device_copy": 4.56, "float4_copy_kernel": 6.3}  # DESIGN 8 item 3 (tools/gpu.sh bw)


def one_call(ctx, genome, regions, params):
    """(wall ms, kernels ms, candidates, plane bytes read) of one vsc_guides_enumerate; the result is freed"""
    L = va.lib()
    h = C.c_void_p()
    t0 = time.perf_counter()
    _lib.check(L.vsc_guides_enumerate(ctx._h, genome._h, regions._h if regions is not None else None, C.byref(params), C.byref(h)),
               ctx._h)
    wall = (time.perf_counter() - t0) * 1e3
    n = int(L.vsc_guides_count(h))
    L.vsc_guides_free(h)
    t = ctx.timing()
    assert t["sites"] == n
    return wall, t["scan_ms"], n, t["genome_bytes"]


def measure(ctx, genome, regions, params, calls, warmup):
    for _ in range(warmup):
        one_call(ctx, genome, regions, params)
    return summarize([one_call(ctx, genome, regions, params) for _ in range(calls)])


def one_pattern_call(ctx, genome, pattern, params, targets):
    """(wall ms, kernels ms, candidates, plane bytes read) of one vsc_guides_enumerate_pattern; the result is freed"""
    L = va.lib()
    h = C.c_void_p()
    t0 = time.perf_counter()
    _lib.check(L.vsc_guides_enumerate_pattern(ctx._h, genome._h, pattern.encode(), len(pattern), C.byref(params),
                                              _lib.ptr(targets), 0 if targets is None else len(targets), C.byref(h)), ctx._h)
    wall = (time.perf_counter() - t0) * 1e3
    n = int(L.vsc_pattern_guides_count(h))
    L.vsc_pattern_guides_free(h)
    t = ctx.timing()
    assert t["sites"] == n
    return wall, t["scan_ms"], n, t["genome_bytes"]


def summarize(runs):
    """The report over the runs of either call: (wall ms, kernels ms, candidates, plane bytes read) each."""
    assert len({(r[2], r[3]) for r in runs}) == 1
    n, plane_bytes = runs[0][2], runs[0][3]
    floor = plane_bytes + 24 * n
    kernel = sorted(r[1] for r in runs)
    out = {"candidates": n, "plane_bytes_read": plane_bytes, "floor_bytes": floor, "kernels_ms": kernel, "wall_ms": sorted(r[0] for r in runs),
           "floor_tb_per_s_at_fastest": floor / (kernel[0] * 1e-3) / 1e12 if kernel[0] > 0 else None}
    for name, tbs in COPY_TBS.items():
        out["floor_ms_at_" + name] = floor / (tbs * 1e12) * 1e3
        out["share_of_" + name] = (floor / (kernel[0] * 1e-3) / 1e12) / tbs if kernel[0] > 0 else None
    return out


def measure_pattern(ctx, genome, pattern, params, targets, calls, warmup):
    for _ in range(warmup):
        one_pattern_call(ctx, genome, pattern, params, targets)
    return dict(summarize([one_pattern_call(ctx, genome, pattern, params, targets) for _ in range(calls)]), pattern=pattern,
                protospacer=[int(params.ps_start), int(params.ps_len)])


PATTERN_CASES = ("spcas9", "sacas9", "cas12a", "spcas9_gc_t", "exons")


def run_pattern_cases(ctx, genome, table, args, res):
    from varscot_amd.api import _pattern_enum_params
    want = PATTERN_CASES if args.pattern_case == "all" else (args.pattern_case,)
    sp = "N" * 21 + "GG"

    def report(key, value):
        res["cases"][key] = value
        print(json.dumps({key: value}), flush=True)

    if "spcas9" in want:
        mine = measure_pattern(ctx, genome, sp, _pattern_enum_params((0, 20), "overlap", "both", (0, 0), 0, 0), None, args.calls, args.warmup)
        report("pattern_spcas9", mine)
        theirs = measure(ctx, genome, None, _enum_params("GG", "both", (0, 0), 0, 0), args.calls, args.warmup)
        assert theirs["candidates"] == mine["candidates"]
        report("guides_enumerate_NGG", theirs)
        report("pattern_over_guides_enumerate", {"kernels_ms_fastest": mine["kernels_ms"][0] / theirs["kernels_ms"][0],
                                                 "kernels_ms_slowest": mine["kernels_ms"][-1] / theirs["kernels_ms"][-1]})
    for key, preset in (("sacas9", "SaCas9"), ("cas12a", "Cas12a")):
        if key in want:
            pattern, _ = va.pattern_strings(preset)
            p = _pattern_enum_params(va.pattern_protospacer(preset), "overlap", "both", (0, 0), 0, 0)
            report("pattern_" + key, measure_pattern(ctx, genome, pattern, p, None, args.calls, args.warmup))
    if "spcas9_gc_t" in want:
        p = _pattern_enum_params((0, 20), "overlap", "both", (8, 14), 3, 0)
        report("pattern_spcas9_gc8-14_t3", measure_pattern(ctx, genome, sp, p, None, args.calls, args.warmup))
    if "exons" in want:
        iv = synth.synthetic_regions(table, args.intervals, args.fraction)
        for rule in ("overlap", "inside"):
            p = _pattern_enum_params((0, 20), rule, "both", (0, 0), 0, 0)
            report("pattern_spcas9_exons_" + rule, dict(measure_pattern(ctx, genome, sp, p, iv, args.calls, args.warmup),
                                                        intervals=args.intervals, fraction=args.fraction))


def measure_locate(ctx, genome, regions, params, calls, warmup):
    """vsc_guides_locate over the candidates of `regions`, labelled against `regions`"""
    L = va.lib()
    h = C.c_void_p()
    _lib.check(L.vsc_guides_enumerate(ctx._h, genome._h, regions._h, C.byref(params), C.byref(h)), ctx._h)
    n = int(L.vsc_guides_count(h))
    labels = np.empty(n, dtype=np.uint32)

    def call():
        t0 = time.perf_counter()
        _lib.check(L.vsc_guides_locate(h, regions._h, _lib.ptr(labels)), ctx._h)
        return (time.perf_counter() - t0) * 1e3

    L.vsc_debug_set_host_timing(1)
    first = call()
    for _ in range(warmup):
        call()
    wall = sorted(call() for _ in range(calls))
    L.vsc_debug_set_host_timing(0)
    L.vsc_guides_free(h)
    floor = 20 * n
    out = {"records": n, "labelled": int((labels != va.REGION_NONE).sum()), "floor_bytes": floor, "first_call_ms": first,
           "wall_ms": wall, "upload_bytes": 12 * regions.info()["intervals"]}
    for name, tbs in COPY_TBS.items():
        out["floor_ms_at_" + name] = floor / (tbs * 1e12) * 1e3
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--case", default="both", choices=["genome", "regions", "both"])
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--intervals", type=int, default=250_000)
    ap.add_argument("--fraction", type=float, default=0.03)
    ap.add_argument("--locate", action="store_true", help="time vsc_guides_locate over the exon-like candidates instead")
    ap.add_argument("--pattern", action="store_true", help="time vsc_guides_enumerate_pattern instead")
    ap.add_argument("--pattern-case", default="all", choices=("all",) + PATTERN_CASES, help="with --pattern: one case alone")
    ap.add_argument("--out", default=None, help="default: profiles/enumerate.json (--locate: profiles/locate.json, --pattern: profiles/pattern_enum.json)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "locate.json" if args.locate else "pattern_enum.json" if args.pattern else "enumerate.json")
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    res = {"genome_bases": args.bases, "calls": args.calls, "warmup": args.warmup, "copy_tb_per_s": COPY_TBS, "cases": {}}
    plain = _enum_params("GG", "both", (0, 0), 0, 0)
    if args.pattern:
        args.case = "pattern"
        run_pattern_cases(ctx, genome, table, args, res)
    elif args.locate:
        args.case = "locate"
        iv = synth.synthetic_regions(table, args.intervals, args.fraction)
        regions = va.Regions(va.PackedGenome(None, None, None, table), iv, rule="overlap")
        res["cases"]["guides_locate_overlap"] = dict(measure_locate(ctx, genome, regions, plain, args.calls, args.warmup),
                                                     intervals=args.intervals, fraction=args.fraction)
        print(json.dumps(res["cases"]), flush=True)
        regions.close()
    if args.case in ("genome", "both"):
        res["cases"]["genome_NGG_both_strands"] = measure(ctx, genome, None, plain, args.calls, args.warmup)
        print(json.dumps({"genome_NGG_both_strands": res["cases"]["genome_NGG_both_strands"]}), flush=True)
    if args.case in ("regions", "both"):
        iv = synth.synthetic_regions(table, args.intervals, args.fraction)
        strict = _enum_params("GG", "both", (8, 14), 3, 0)
        for rule in ("overlap", "inside"):
            regions = va.Regions(va.PackedGenome(None, None, None, table), iv, rule=rule)
            for label, p in (("", plain), ("_gc8-14_t3", strict)):
                key = "regions_%s%s" % (rule, label)
                res["cases"][key] = dict(measure(ctx, genome, regions, p, args.calls, args.warmup), intervals=args.intervals,
                                         fraction=args.fraction, info=regions.info())
                print(json.dumps({key: res["cases"][key]}), flush=True)
            regions.close()
    genome.close()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

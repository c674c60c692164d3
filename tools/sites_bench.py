"""Cut sites (vsc_hits_sites) on the synthetic hg38-sized genome of varscot_amd.synth, one GPU - tools/bulge_bench.py's genome
and guides.

    python tools/sites_bench.py                         both cases, JSON to profiles/sites.json (and stdout)

16 synthetic guides at 4 mismatches, the cases -u 1,1 and -u 2,2.  Every case, after W warm-up rounds, K timed rounds, fastest ..
slowest:
  (the plain search runs with VSC_ALGO_SCAN, as in tools/bulge_bench.py: no seed index is built)
  kernels      the collapse's stages between HIP events on the context's stream (vsc_debug_sites_ms): flag pass + scan, write
               pass - beside the kernels of the two searches they follow (vsc_timing.scan_ms / total_ms of vsc_search and of
               vsc_search_bulges), over results that stay on the device;
  collapse     host wall time of the one vsc_hits_sites call (records and rows, its read-back and the rows' copy included);
  device route host wall time of Genome.search_sites: the two searches, the collapse, the sites copied out;
  host route   host wall time of the two searches, BOTH record lists copied out, and vsc_sites_collapse on the host.
The two routes' records and rows are compared byte for byte.  Reported with the record and site counts.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import varscot_amd as va  # noqa: E402
from varscot_amd import _lib, dist as vdist, synth  # noqa: E402


def searches(ctx, genome, codes, m, dna, rna):
    """(plain handle, bulged handle, timings of the two searches); both results stay on the device"""
    L = va.lib()
    p = genome._params(m, None, "scan")
    plain, bulged = C.c_void_p(), C.c_void_p()
    _lib.check(L.vsc_search(ctx._h, genome._h, _lib.ptr(codes), len(codes), C.byref(p), C.byref(plain)), ctx._h)
    tp = ctx.timing()
    pb = genome._params(m, None, "scan")
    bp = _lib.BulgeParams(dna, rna, 0, 0, 0)
    _lib.check(L.vsc_search_bulges(ctx._h, genome._h, _lib.ptr(codes), len(codes), C.byref(pb), C.byref(bp), C.byref(bulged), None), ctx._h)
    tb = ctx.timing()
    return plain, bulged, tp, tb


def free(plain, bulged):
    va.lib().vsc_bulge_hits_free(bulged)
    va.lib().vsc_hits_free(plain)


def kernels_round(ctx, genome, codes, m, dna, rna):
    L = va.lib()
    plain, bulged, tp, tb = searches(ctx, genome, codes, m, dna, rna)
    try:
        p = _lib.SiteParams(23, _lib.SITE_ANCHOR_END)
        rows = np.zeros(len(codes), dtype=va.SITE_ROW_DTYPE)
        h = C.c_void_p()
        t0 = time.perf_counter()
        _lib.check(L.vsc_hits_sites(ctx._h, plain, bulged, len(codes), C.byref(p), C.byref(h), _lib.ptr(rows)), ctx._h)
        wall = (time.perf_counter() - t0) * 1e3
        flag, write = C.c_double(0), C.c_double(0)
        _lib.check(L.vsc_debug_sites_ms(ctx._h, C.byref(flag), C.byref(write)), ctx._h)
        n = int(L.vsc_sites_count(h))
        L.vsc_sites_free(h)
        assert n == int(rows["sites"].sum())
        return {"flag_scan_ms": flag.value, "write_ms": write.value, "collapse_wall_ms": wall, "plain_search_total_ms": tp["total_ms"],
                "plain_search_algorithm": tp["algorithm"], "bulge_search_kernels_ms": tb["scan_ms"], "plain_records": int(L.vsc_hits_count(plain)),
                "bulged_records": int(L.vsc_bulge_hits_count(bulged)), "sites": n, "bulge_only": int(rows["bulge_only"].sum()),
                "sites_by_size_and_nm": rows["count"].sum(0).tolist()}
    finally:
        free(plain, bulged)


def device_route(genome, codes, m, dna, rna):
    t0 = time.perf_counter()
    got = genome.search_sites(codes, m, dna=dna, rna=rna, algorithm="scan")
    return (time.perf_counter() - t0) * 1e3, got


def host_route(ctx, genome, codes, m, dna, rna):
    L = va.lib()
    t0 = time.perf_counter()
    plain, bulged, _, _ = searches(ctx, genome, codes, m, dna, rna)
    try:
        recs = []
        for h, count, data, dtype in ((plain, L.vsc_hits_count, L.vsc_hits_data, va.HIT_DTYPE),
                                      (bulged, L.vsc_bulge_hits_count, L.vsc_bulge_hits_data, va.BULGE_HIT_DTYPE)):
            n, d = int(count(h)), C.c_void_p()
            _lib.check(data(h, C.byref(d)), ctx._h)
            recs.append(np.frombuffer((C.c_char * (n * 16)).from_address(d.value), dtype=dtype).copy() if n else np.zeros(0, dtype=dtype))
        got = va.collapse_sites(recs[0], recs[1], len(codes))
    finally:
        free(plain, bulged)
    return (time.perf_counter() - t0) * 1e3, got


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--guides", type=int, default=16)
    ap.add_argument("--mismatches", type=int, default=4)
    ap.add_argument("--bases", type=int, default=3_000_000_000, help="genome size (default: the hg38-sized synthetic genome)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sites.json"))
    args = ap.parse_args()
    table, _ = synth.contig_table(args.bases)
    span = int(table[-1]["offset"]) + int(table[-1]["length"]) + 1
    n_words = (span + 31) // 32
    wb, we = vdist.shard_words(n_words, 0, 1)
    hi, lo, nm, _, _, _ = synth.synthetic_planes(args.bases, wb, min(we + 1, n_words))
    ctx = va.Context(0)
    genome = va.Genome.from_shard(ctx, hi, lo, nm, wb, we - wb, table)
    del hi, lo, nm
    codes = va.pack_guides(synth.synthetic_guides(args.guides)[1])
    m = args.mismatches
    res = {"genome_bases": args.bases, "guides": args.guides, "mismatches": m, "calls": args.calls, "warmup": args.warmup, "cases": {}}
    for dna, rna in ((1, 1), (2, 2)):
        for _ in range(args.warmup):
            kernels_round(ctx, genome, codes, m, dna, rna)
            device_route(genome, codes, m, dna, rna)
            host_route(ctx, genome, codes, m, dna, rna)
        rounds = [kernels_round(ctx, genome, codes, m, dna, rna) for _ in range(args.calls)]
        dev = [device_route(genome, codes, m, dna, rna) for _ in range(args.calls)]
        host = [host_route(ctx, genome, codes, m, dna, rna) for _ in range(args.calls)]
        for _, got in dev + host:
            assert got[0].tobytes() == dev[0][1][0].tobytes() and got[1].tobytes() == dev[0][1][1].tobytes()
        case = {k: rounds[0][k] for k in ("plain_records", "bulged_records", "sites", "bulge_only", "sites_by_size_and_nm", "plain_search_algorithm")}
        for k in ("flag_scan_ms", "write_ms", "collapse_wall_ms", "plain_search_total_ms", "bulge_search_kernels_ms"):
            case[k] = sorted(r[k] for r in rounds)
        case["device_route_wall_ms"] = sorted(r[0] for r in dev)
        case["host_route_wall_ms"] = sorted(r[0] for r in host)
        case["alignments_per_site"] = (case["plain_records"] + case["bulged_records"]) / max(case["sites"], 1)
        res["cases"]["u%d,%d" % (dna, rna)] = case
        print(json.dumps({"u%d,%d" % (dna, rna): case}), flush=True)
    genome.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

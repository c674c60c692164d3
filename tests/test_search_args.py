"""The argument checks of every search entry point: one rejected call per entry point and mistake, made through the C ABI
directly (varscot_amd.api would refuse most of them first), with the return code and the exact text of vsc_last_error /
vsc_multi_last_error.  Every rejection comes from a host-side check; no search kernel runs.

EXPECTED was recorded from the library before the search calls were moved onto one pass loop, and holds unchanged since:
where two entry points word the same mistake differently, it says so."""
import ctypes as C

import numpy as np
import pytest

import varscot_amd as va
from helpers import random_guides, random_seq
from varscot_amd import _lib

pytestmark = pytest.mark.gpu

# the arguments of every entry point, in call order
_SEARCH = ("handle", "genome", "guides", "n", "params")
ENTRY_POINTS = {
    "vsc_search": _SEARCH + ("hits",),
    "vsc_search_summary": _SEARCH + ("exclude", "out"),
    "vsc_search_summary_regions": _SEARCH + ("exclude", "regions", "out", "out_in"),
    "vsc_search_select": _SEARCH + ("select", "exclude", "summary", "hits"),
    "vsc_search_select_regions": _SEARCH + ("select", "filter", "exclude", "summary", "summary_in", "hits"),
    "vsc_search_stream": _SEARCH + ("batch", "callback", "user"),
    "vsc_search_stream_rows": _SEARCH + ("batch", "callback", "user"),
    "vsc_multi_search": _SEARCH + ("hits",),
    "vsc_multi_search_summary": _SEARCH + ("exclude", "out"),
    "vsc_multi_search_summary_regions": _SEARCH + ("exclude", "regions", "out", "out_in"),
    "vsc_multi_search_select": _SEARCH + ("select", "exclude", "summary", "hits"),
    "vsc_multi_search_select_regions": _SEARCH + ("select", "filter", "exclude", "summary", "summary_in", "hits"),
    "vsc_multi_search_stream": _SEARCH + ("batch", "score", "callback", "user"),
}
# mistake -> the argument (or one of the arguments) an entry point must take for the mistake to be one there; `out` and
# `out_in` are the rows a summary call must be given, `summary` and `summary_in` the optional ones of a select call
MISTAKES = {
    "null params": "params",
    "null guides": "guides",
    "genome of another context": "genome",
    "9 mismatches": "params",
    "unknown algorithm": "params",
    "null callback": "callback",
    "null select": "select",
    "select reserved": "select",
    "filter without regions": "filter",
    "filter scope 2": "filter",
    "summary_in without filter": "filter",
    "regions of another table": ("regions", "filter"),
    "excluded contig": "exclude",
    "excluded strand 2": "exclude",
    "null out": "out",
    "null out_in": "out_in",
    "unknown scoring mode": "score",
    "votes without model": "score",
    # two mistakes at once: which check comes first
    "null callback and null params": "callback",
    "null select and unknown algorithm": "select",
    "filter scope 2 and null params": "filter",
}


def applies(entry, mistake):
    args, need = ENTRY_POINTS[entry], MISTAKES[mistake]
    return any(a in args for a in ((need,) if isinstance(need, str) else need))


CASES = [(e, m) for e in ENTRY_POINTS for m in MISTAKES if applies(e, m)]

# (entry point, mistake) -> (return code, error text)
EXPECTED = {
    ('vsc_search', 'null params'): (-22, 'vsc_search: null argument'),
    ('vsc_search', 'null guides'): (-22, 'vsc_search: null argument'),
    ('vsc_search', 'genome of another context'): (-22, 'vsc_search: genome belongs to another context'),
    ('vsc_search', '9 mismatches'): (-22, 'Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_search', 'unknown algorithm'): (-22, 'vsc_search: unknown algorithm'),
    ('vsc_search_summary', 'null params'): (-22, 'vsc_search_summary: null argument'),
    ('vsc_search_summary', 'null guides'): (-22, 'vsc_search_summary: null argument'),
    ('vsc_search_summary', 'genome of another context'): (-22, 'vsc_search_summary: genome belongs to another context'),
    ('vsc_search_summary', '9 mismatches'): (-22, 'Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_search_summary', 'unknown algorithm'): (-22, 'vsc_search_summary: unknown algorithm'),
    ('vsc_search_summary', 'excluded contig'): (-22, "vsc_search_summary: excluded locus outside the genome's contigs or strands"),
    ('vsc_search_summary', 'excluded strand 2'): (-22, "vsc_search_summary: excluded locus outside the genome's contigs or strands"),
    ('vsc_search_summary', 'null out'): (-22, 'vsc_search_summary: null argument'),
    ('vsc_search_summary_regions', 'null params'): (-22, 'vsc_search_summary_regions: null argument'),
    ('vsc_search_summary_regions', 'null guides'): (-22, 'vsc_search_summary_regions: null argument'),
    ('vsc_search_summary_regions', 'genome of another context'): (-22, 'vsc_search_summary_regions: genome belongs to another context'),
    ('vsc_search_summary_regions', '9 mismatches'): (-22, 'Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_search_summary_regions', 'unknown algorithm'): (-22, 'vsc_search_summary_regions: unknown algorithm'),
    ('vsc_search_summary_regions', 'regions of another table'): (-22, 'vsc_search_summary_regions: the regions were built for another contig table'),
    ('vsc_search_summary_regions', 'excluded contig'): (-22, "vsc_search_summary_regions: excluded locus outside the genome's contigs or strands"),
    ('vsc_search_summary_regions', 'excluded strand 2'): (-22, "vsc_search_summary_regions: excluded locus outside the genome's contigs or strands"),
    ('vsc_search_summary_regions', 'null out'): (-22, 'vsc_search_summary_regions: null argument'),
    ('vsc_search_summary_regions', 'null out_in'): (-22, 'vsc_search_summary_regions: null argument'),
    ('vsc_search_select', 'null params'): (-22, 'vsc_search_select: null argument'),
    ('vsc_search_select', 'null guides'): (-22, 'vsc_search_select: null argument'),
    ('vsc_search_select', 'genome of another context'): (-22, 'vsc_search_select: genome belongs to another context'),
    ('vsc_search_select', '9 mismatches'): (-22, 'Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_search_select', 'unknown algorithm'): (-22, 'vsc_search_select: unknown algorithm'),
    ('vsc_search_select', 'null select'): (-22, 'vsc_search_select: null argument'),
    ('vsc_search_select', 'select reserved'): (-22, 'vsc_search_select: reserved fields must be 0'),
    ('vsc_search_select', 'excluded contig'): (-22, "vsc_search_select: excluded locus outside the genome's contigs or strands"),
    ('vsc_search_select', 'excluded strand 2'): (-22, "vsc_search_select: excluded locus outside the genome's contigs or strands"),
    ('vsc_search_select_regions', 'null params'): (-22, 'vsc_search_select_regions: null argument'),
    ('vsc_search_select_regions', 'null guides'): (-22, 'vsc_search_select_regions: null argument'),
    ('vsc_search_select_regions', 'genome of another context'): (-22, 'vsc_search_select_regions: genome belongs to another context'),
    ('vsc_search_select_regions', '9 mismatches'): (-22, 'Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_search_select_regions', 'unknown algorithm'): (-22, 'vsc_search_select_regions: unknown algorithm'),
    ('vsc_search_select_regions', 'null select'): (-22, 'vsc_search_select_regions: null argument'),
    ('vsc_search_select_regions', 'select reserved'): (-22, 'vsc_search_select_regions: reserved fields must be 0'),
    ('vsc_search_select_regions', 'filter without regions'): (-22, 'vsc_search_select_regions: a filter needs regions, a scope of 0 or 1 and a reserved field of 0'),
    ('vsc_search_select_regions', 'filter scope 2'): (-22, 'vsc_search_select_regions: a filter needs regions, a scope of 0 or 1 and a reserved field of 0'),
    ('vsc_search_select_regions', 'summary_in without filter'): (-22, 'vsc_search_select_regions: summary_in without a filter'),
    ('vsc_search_select_regions', 'regions of another table'): (-22, 'vsc_search_select_regions: the regions were built for another contig table'),
    ('vsc_search_select_regions', 'excluded contig'): (-22, "vsc_search_select_regions: excluded locus outside the genome's contigs or strands"),
    ('vsc_search_select_regions', 'excluded strand 2'): (-22, "vsc_search_select_regions: excluded locus outside the genome's contigs or strands"),
    ('vsc_search_stream', 'null params'): (-22, 'vsc_search_stream: null argument'),
    ('vsc_search_stream', 'null guides'): (-22, 'vsc_search_stream: null argument'),
    ('vsc_search_stream', 'genome of another context'): (-22, 'vsc_search_stream: genome belongs to another context'),
    ('vsc_search_stream', '9 mismatches'): (-22, 'Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_search_stream', 'unknown algorithm'): (-22, 'vsc_search_stream: unknown algorithm'),
    ('vsc_search_stream', 'null callback'): (-22, 'vsc_search_stream: null callback'),
    ('vsc_search_stream_rows', 'null params'): (-22, 'vsc_search_stream_rows: null argument'),
    ('vsc_search_stream_rows', 'null guides'): (-22, 'vsc_search_stream_rows: null argument'),
    ('vsc_search_stream_rows', 'genome of another context'): (-22, 'vsc_search_stream_rows: genome belongs to another context'),
    ('vsc_search_stream_rows', '9 mismatches'): (-22, 'Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_search_stream_rows', 'unknown algorithm'): (-22, 'vsc_search_stream_rows: unknown algorithm'),
    ('vsc_search_stream_rows', 'null callback'): (-22, 'vsc_search_stream_rows: null callback'),
    ('vsc_multi_search', 'null params'): (-22, 'vsc_multi_search: null argument'),
    ('vsc_multi_search', 'null guides'): (-22, 'vsc_multi_search: null argument'),
    ('vsc_multi_search', 'genome of another context'): (-22, 'vsc_multi_search: null argument'),
    ('vsc_multi_search', '9 mismatches'): (-22, 'shard 0: Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_multi_search', 'unknown algorithm'): (-22, 'shard 0: vsc_search: unknown algorithm'),
    ('vsc_multi_search_summary', 'null params'): (-22, 'vsc_multi_search_summary: null argument'),
    ('vsc_multi_search_summary', 'null guides'): (-22, 'vsc_multi_search_summary: null argument'),
    ('vsc_multi_search_summary', 'genome of another context'): (-22, 'vsc_multi_search_summary: null argument'),
    ('vsc_multi_search_summary', '9 mismatches'): (-22, 'shard 0: Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_multi_search_summary', 'unknown algorithm'): (-22, 'shard 0: vsc_search_summary: unknown algorithm'),
    ('vsc_multi_search_summary', 'excluded contig'): (-22, "vsc_multi_search_summary: excluded locus outside the genome's contigs or strands"),
    ('vsc_multi_search_summary', 'excluded strand 2'): (-22, "vsc_multi_search_summary: excluded locus outside the genome's contigs or strands"),
    ('vsc_multi_search_summary', 'null out'): (-22, 'vsc_multi_search_summary: null argument'),
    ('vsc_multi_search_summary_regions', 'null params'): (-22, 'vsc_multi_search_summary_regions: null argument'),
    ('vsc_multi_search_summary_regions', 'null guides'): (-22, 'vsc_multi_search_summary_regions: null argument'),
    ('vsc_multi_search_summary_regions', 'genome of another context'): (-22, 'vsc_multi_search_summary_regions: null argument'),
    ('vsc_multi_search_summary_regions', '9 mismatches'): (-22, 'shard 0: Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_multi_search_summary_regions', 'unknown algorithm'): (-22, 'shard 0: vsc_search_summary_regions: unknown algorithm'),
    ('vsc_multi_search_summary_regions', 'regions of another table'): (-22, 'shard 0: vsc_search_summary_regions: the regions were built for another contig table'),
    ('vsc_multi_search_summary_regions', 'excluded contig'): (-22, "vsc_multi_search_summary_regions: excluded locus outside the genome's contigs or strands"),
    ('vsc_multi_search_summary_regions', 'excluded strand 2'): (-22, "vsc_multi_search_summary_regions: excluded locus outside the genome's contigs or strands"),
    ('vsc_multi_search_summary_regions', 'null out'): (-22, 'vsc_multi_search_summary_regions: null argument'),
    ('vsc_multi_search_summary_regions', 'null out_in'): (-22, 'vsc_multi_search_summary_regions: null argument'),
    ('vsc_multi_search_select', 'null params'): (-22, 'vsc_multi_search_select: null argument'),
    ('vsc_multi_search_select', 'null guides'): (-22, 'vsc_multi_search_select: null argument'),
    ('vsc_multi_search_select', 'genome of another context'): (-22, 'vsc_multi_search_select: null argument'),
    ('vsc_multi_search_select', '9 mismatches'): (-22, 'shard 0: Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_multi_search_select', 'unknown algorithm'): (-22, 'shard 0: vsc_search_select: unknown algorithm'),
    ('vsc_multi_search_select', 'null select'): (-22, 'vsc_multi_search_select: null argument'),
    ('vsc_multi_search_select', 'select reserved'): (-22, 'vsc_multi_search_select: reserved fields must be 0'),
    ('vsc_multi_search_select', 'excluded contig'): (-22, "vsc_multi_search_select: excluded locus outside the genome's contigs or strands"),
    ('vsc_multi_search_select', 'excluded strand 2'): (-22, "vsc_multi_search_select: excluded locus outside the genome's contigs or strands"),
    ('vsc_multi_search_select_regions', 'null params'): (-22, 'vsc_multi_search_select_regions: null argument'),
    ('vsc_multi_search_select_regions', 'null guides'): (-22, 'vsc_multi_search_select_regions: null argument'),
    ('vsc_multi_search_select_regions', 'genome of another context'): (-22, 'vsc_multi_search_select_regions: null argument'),
    ('vsc_multi_search_select_regions', '9 mismatches'): (-22, 'shard 0: Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_multi_search_select_regions', 'unknown algorithm'): (-22, 'shard 0: vsc_search_select_regions: unknown algorithm'),
    ('vsc_multi_search_select_regions', 'null select'): (-22, 'vsc_multi_search_select_regions: null argument'),
    ('vsc_multi_search_select_regions', 'select reserved'): (-22, 'vsc_multi_search_select_regions: reserved fields must be 0'),
    ('vsc_multi_search_select_regions', 'filter without regions'): (-22, 'vsc_multi_search_select_regions: a filter needs regions, a scope of 0 or 1 and a reserved field of 0'),
    ('vsc_multi_search_select_regions', 'filter scope 2'): (-22, 'vsc_multi_search_select_regions: a filter needs regions, a scope of 0 or 1 and a reserved field of 0'),
    ('vsc_multi_search_select_regions', 'summary_in without filter'): (-22, 'vsc_multi_search_select_regions: summary_in without a filter'),
    ('vsc_multi_search_select_regions', 'regions of another table'): (-22, 'shard 0: vsc_search_select_regions: the regions were built for another contig table'),
    ('vsc_multi_search_select_regions', 'excluded contig'): (-22, "vsc_multi_search_select_regions: excluded locus outside the genome's contigs or strands"),
    ('vsc_multi_search_select_regions', 'excluded strand 2'): (-22, "vsc_multi_search_select_regions: excluded locus outside the genome's contigs or strands"),
    ('vsc_multi_search_stream', 'null params'): (-22, 'vsc_multi_search_stream: null argument'),
    ('vsc_multi_search_stream', 'null guides'): (-22, 'vsc_multi_search_stream: null argument'),
    ('vsc_multi_search_stream', 'genome of another context'): (-22, 'vsc_multi_search_stream: null argument'),
    ('vsc_multi_search_stream', '9 mismatches'): (-22, 'shard 0: Maximum number of mismatches must lie between 0 and 8.'),
    ('vsc_multi_search_stream', 'unknown algorithm'): (-22, 'shard 0: vsc_search: unknown algorithm'),
    ('vsc_multi_search_stream', 'null callback'): (-22, 'vsc_multi_search_stream: null argument'),
    ('vsc_multi_search_stream', 'unknown scoring mode'): (-22, 'vsc_multi_search_stream: unknown scoring mode'),
    ('vsc_multi_search_stream', 'votes without model'): (-22, "vsc_multi_search_stream: the votes need a forest and the reads' activities"),
    # two mistakes at once: which check comes first
    ('vsc_search_stream', 'null callback and null params'): (-22, 'vsc_search_stream: null argument'),
    ('vsc_search_stream_rows', 'null callback and null params'): (-22, 'vsc_search_stream_rows: null argument'),
    ('vsc_multi_search_stream', 'null callback and null params'): (-22, 'vsc_multi_search_stream: null argument'),
    ('vsc_search_select', 'null select and unknown algorithm'): (-22, 'vsc_search_select: unknown algorithm'),
    ('vsc_search_select_regions', 'null select and unknown algorithm'): (-22, 'vsc_search_select_regions: unknown algorithm'),
    ('vsc_multi_search_select', 'null select and unknown algorithm'): (-22, 'vsc_multi_search_select: null argument'),
    ('vsc_multi_search_select_regions', 'null select and unknown algorithm'): (-22, 'vsc_multi_search_select_regions: null argument'),
    ('vsc_search_select_regions', 'filter scope 2 and null params'): (-22, 'vsc_search_select_regions: a filter needs regions, a scope of 0 or 1 and a reserved field of 0'),
    ('vsc_multi_search_select_regions', 'filter scope 2 and null params'): (-22, 'vsc_multi_search_select_regions: null argument'),
}


class World:
    """A context with a genome of a few hundred bases, a second context with its own copy (the foreign genome), the same
    pair as one-device vsc_multi objects, and regions for the genome's contig table and for another one."""

    def __init__(self):
        rng = np.random.default_rng(77)
        contigs = [random_seq(rng, 300), random_seq(rng, 120)]
        self.packed = va.PackedGenome.from_sequences(contigs)
        self.codes = va.pack_guides(random_guides(rng, 3))
        self.ctx, self.other_ctx = va.Context(0), va.Context(0)
        self.genome, self.other_genome = self.ctx.load_genome(self.packed), self.other_ctx.load_genome(self.packed)
        self.multi, self.other_multi = va.MultiContext([0]), va.MultiContext([0])
        self.multi_genome, self.other_multi_genome = self.multi.load_genome(self.packed), self.other_multi.load_genome(self.packed)
        self.regions = va.Regions(self.packed, [(0, 10, 90), (1, 0, 50)])
        self.other_regions = va.Regions(va.PackedGenome.from_sequences([random_seq(rng, 200)]), [(0, 10, 90)])
        self.n_contigs = len(contigs)

    def close(self):
        for o in (self.regions, self.other_regions, self.multi, self.other_multi, self.ctx, self.other_ctx):
            o.close()

    def valid(self, entry):
        """Arguments `entry` accepts, by name (and those of the other entry points, which it does not take)."""
        multi, n = entry.startswith("vsc_multi_"), len(self.codes)
        callback = {"vsc_search_stream": _lib.BATCH_FN, "vsc_search_stream_rows": _lib.ROWS_BATCH_FN,
                    "vsc_multi_search_stream": _lib.MULTI_BATCH_FN}.get(entry)
        return dict(handle=self.multi._h if multi else self.ctx._h, genome=self.multi_genome._h if multi else self.genome._h,
                    guides=self.codes, n=n, params=_lib.SearchParams(4, 0, b"", _lib.ALGO_AUTO), hits=C.c_void_p(), exclude=None,
                    regions=self.regions._h, out=self.rows(), out_in=self.rows(), summary=None, summary_in=None,
                    select=_lib.Select(2, 0), filter=_lib.RegionFilter(self.regions._h, _lib.REGION_KEEP, 0), batch=0, score=None,
                    callback=callback(lambda *unused: 0) if callback else None, user=None)

    def rows(self):
        return np.zeros(len(self.codes), dtype=_lib.SUMMARY_DTYPE)

    def loci(self, contig, strand):
        """No excluded locus but the second read's."""
        ex = np.zeros(len(self.codes), dtype=_lib.LOCUS_DTYPE)
        ex["contig"] = 0xFFFFFFFF
        ex["contig"][1], ex["strand"][1] = contig, strand
        return ex

    def spoil(self, a, mistake, multi):
        if mistake == "null params":
            a["params"] = None
        elif mistake == "null guides":
            a["guides"] = None
        elif mistake == "genome of another context":
            a["genome"] = self.other_multi_genome._h if multi else self.other_genome._h
        elif mistake == "9 mismatches":
            a["params"].max_mismatches = 9
        elif mistake == "unknown algorithm":
            a["params"].algorithm = 3
        elif mistake == "null callback":
            a["callback"] = type(a["callback"])()  # (a null function pointer)
        elif mistake == "null select":
            a["select"] = None
        elif mistake == "select reserved":
            a["select"].reserved[1] = 1
        elif mistake == "filter without regions":
            a["filter"] = _lib.RegionFilter(None, _lib.REGION_KEEP, 0)
        elif mistake == "filter scope 2":
            a["filter"] = _lib.RegionFilter(self.regions._h, 2, 0)
        elif mistake == "summary_in without filter":
            a["filter"], a["summary_in"] = None, self.rows()
        elif mistake == "regions of another table":
            a["regions"], a["filter"] = self.other_regions._h, _lib.RegionFilter(self.other_regions._h, _lib.REGION_KEEP, 0)
        elif mistake == "excluded contig":
            a["exclude"] = self.loci(self.n_contigs, 0)
        elif mistake == "excluded strand 2":
            a["exclude"] = self.loci(0, 2)
        elif mistake == "null out":
            a["out"] = None
        elif mistake == "null out_in":
            a["out_in"] = None
        elif mistake == "unknown scoring mode":
            a["score"] = _lib.MultiScore(3, 0, None, None)
        elif mistake == "votes without model":
            a["activity"] = np.ones(len(self.codes), dtype=np.float64)
            a["score"] = _lib.MultiScore(_lib.MULTI_SCORE_VOTES, 0, _lib.ptr(a["activity"]), None)
        else:
            raise KeyError(mistake)

    def call(self, entry, mistake):
        """The call of `entry` with valid arguments but for `mistake`: (return code, error text, hits handle or None)."""
        L, multi = va.lib(), entry.startswith("vsc_multi_")
        a = self.valid(entry)
        for one in mistake.split(" and "):
            self.spoil(a, one, multi)

        def as_arg(name):
            v = a[name]
            if isinstance(v, np.ndarray):
                return _lib.ptr(v)
            if name == "hits" or isinstance(v, C.Structure):
                return C.byref(v)
            return v

        rc = getattr(L, entry)(*[as_arg(name) for name in ENTRY_POINTS[entry]])
        text = (L.vsc_multi_last_error if multi else L.vsc_last_error)(a["handle"]).decode()
        return rc, text, a["hits"].value


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def test_every_case_has_an_expectation():
    assert sorted(EXPECTED) == sorted(CASES)


@pytest.mark.parametrize("entry,mistake", CASES, ids=["%s-%s" % (e, m.replace(" ", "_")) for e, m in CASES])
def test_rejected(world, entry, mistake):
    rc, text, hits = world.call(entry, mistake)
    print(entry, "|", mistake, "->", rc, repr(text))
    assert hits is None  # no result object comes back from a rejected call
    assert (rc, text) == EXPECTED[(entry, mistake)]
    assert rc < 0

"""The host half of the classified sinks (vsc_search_summary_classified / vsc_search_select_classified): the aggregation and the
cut the GPU tests compare against, on hand-made tables; the header's structs; the ABI version.  No device needed."""
import ctypes as C
import os
import re

import numpy as np

import varscot_amd as va
from classified_cases import cut_by_votes, oracle_votes, rows_of_hits, synthetic_forest, votes_rows
from varscot_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "varscot_hip.h")).read()


def test_votes_rows_on_a_hand_made_table():
    # (guide, NM, votes) with 8 trees: active = votes >= 5, tie = votes == 4
    table = [(0, 0, 8), (0, 3, 5), (0, 3, 4), (0, 4, 0), (2, 8, 7), (2, 8, 4), (2, 1, 4), (2, 2, 3)]
    g, nm, v = zip(*table)
    rows = votes_rows(g, nm, v, 4, 8)
    assert rows["votes_sum"].tolist() == [17, 0, 18, 0]
    assert rows["active"].tolist() == [2, 0, 1, 0]
    assert rows["ties"].tolist() == [1, 0, 2, 0]
    assert rows["active_nm"][0].tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0]
    assert rows["active_nm"][2].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert not rows["active_nm"][[1, 3]].any()
    assert va.expected_active(rows, 8).tolist() == [17 / 8, 0.0, 18 / 8, 0.0]
    # an odd tree count has no ties
    assert votes_rows(g, nm, v, 4, 9)["ties"].sum() == 0


def _hits(rows):
    h = np.zeros(len(rows), dtype=va.HIT_DTYPE)
    for i, (g, c, p, strand, nm) in enumerate(rows):
        h[i] = (g, c, p, (strand << 31) | (nm << 23))
    return h


def test_cut_by_votes_order_and_exclusion():
    hits = _hits([(0, 0, 10, 0, 1), (0, 0, 20, 1, 2), (0, 0, 30, 0, 2), (0, 1, 5, 0, 3), (1, 0, 7, 1, 0), (1, 0, 9, 0, 4)])
    votes = [3, 6, 6, 6, 2, 2]
    ranked, v = cut_by_votes(hits, votes, top_k=3, ranked=True)
    # guide 0: three hits share 6 votes - '+' before '-', then the position; guide 1: '+' before '-'
    assert [(int(r["guide"]), int(r["contig"]), int(r["pos"])) for r in ranked] == [(0, 0, 30), (0, 1, 5), (0, 0, 20), (1, 0, 9), (1, 0, 7)]
    assert v.tolist() == [6, 6, 6, 2, 2]
    assert len(cut_by_votes(hits, votes, min_votes=3)) == 4
    ex = [(0, 30, 0), (0xFFFFFFFF, 0, 0)]
    assert [int(p) for p in cut_by_votes(hits, votes, top_k=1, exclude=ex)["pos"]] == [5, 9]
    assert rows_of_hits(hits, votes, 2, 8, exclude=ex)["votes_sum"].tolist() == [15, 4]


def test_header_structs_and_abi_version():
    assert va.lib().vsc_abi_version() == 5 and re.search(r"#define\s+VSC_ABI_VERSION\s+5\b", HEADER)
    m = re.search(r"typedef struct \{([^}]*)\} vsc_guide_votes;", HEADER)
    fields = re.findall(r"uint64_t\s+(\w+)(?:\[(\d+)\])?;", m.group(1))
    assert fields == [("votes_sum", ""), ("active", ""), ("ties", ""), ("active_nm", "9")]
    assert "static_assert(sizeof(vsc_guide_votes) == 96" in HEADER
    assert _lib.VOTES_DTYPE.itemsize == 96 and list(_lib.VOTES_DTYPE.names) == [f for f, _ in fields]
    assert re.search(r"typedef struct \{\s*uint32_t top_k;[^}]*uint32_t min_votes;[^}]*uint32_t reserved\[2\];\s*\} vsc_select_votes;", HEADER)
    assert re.search(r"typedef struct \{\s*const vsc_rf_model \*model;[^}]*const double \*guide_activity;[^}]*uint32_t reserved\[2\];\s*\} vsc_classify;", HEADER)
    assert C.sizeof(_lib.SelectVotes) == 16 and C.sizeof(_lib.Classify) == 24
    for name in ("vsc_search_summary_classified", "vsc_search_select_classified", "vsc_multi_search_summary_classified"):
        assert name in HEADER and getattr(va.lib(), name)


def test_vectorised_oracle_walk_equals_the_oracle(tmp_path):
    from oracle.rf_oracle import Forest as OracleForest
    rng = np.random.default_rng(5)
    path = str(tmp_path / "forest.vscrf")
    synthetic_forest(path, rng, 8, 31)
    of = OracleForest(path)
    rows = np.column_stack([rng.integers(0, 4, size=(50, len(of.names) - 1)), rng.choice([0.2, 0.31, 0.5, 1.02, 1.7], size=50)]).astype(float)
    want = [of.votes(dict(zip(of.names, r))) for r in rows]
    assert oracle_votes(of, rows).tolist() == want and len(set(want)) > 2

"""The scenario of the variant-aware pattern screen (tests/test_pattern_variants_cpu.py, tests/test_pattern_variants.py) and
its restatement: the genome of tests/variants_cases.py's kind - three contigs, one with '_' in its name, planted off-targets on
both strands, 1-4 SNPs / insertions / deletions around three quarters of the sites - for a pattern of any length L, small enough
for the Python oracles.  The oracle side is oracle/variants_oracle.py (the windows, seq_len = L), pattern_cases.brute_force (the
searches), oracle/merge_oracle.get_snp_type(..., L) (the walk), variants_cases.shadows (filterRefAlignment's predicate restated
from merge_results) and pattern_table_cases (the scores); nothing here touches the product."""
import functools

import numpy as np

import pattern_cases as pc
import pattern_table_cases as ptc
from oracle import merge_oracle as mo
from oracle import variants_oracle as vo
from variants_cases import GENOTYPES, shadows, vcf_header

CONTIGS = [("chr1", 24000), ("chr2", 14000), ("chrUn_x", 2500)]
SLOT, SITE_AT = 150, 60  # one site per slot of 150 bases, 60 bases into it: the variants at -30 .. L + 21 stay inside the slot
N_GUIDES, N_PLANTED, N_EDGE = 24, 228, 12
M = 4
SHAPES = {"sa": "N" * 21 + "NNGRRT", "cas12a": "TTTV" + "N" * 23, "sp": "N" * 20 + "NGG", "trunc": "N" * 13 + "NGG",
          "longsa": "N" * 26 + "NNGRRT"}
# chosen on the CPU so that the oracle alone meets FLOORS (test_pattern_variants_cpu.py asserts them)
SEEDS = {"sa": 1, "cas12a": 2, "sp": 1, "trunc": 2, "longsa": 2}
# what every shape of the scenario must hold at M, counted on the oracle's own output (Case.floors)
FLOORS = {"dup_adjacent": 3, "var_records": 3, "dup_apart": 1, "multi_var": 1, "on_target_in_window": 1, "shifted": 1, "shadowed": 1,
          "right_edge": 1, "straddle": 1, "bit0": 1}


def plane_offsets(lengths):
    """Global position of every contig's first base in a packed genome: contigs in order, one separator base between them."""
    off, out = 0, []
    for n in lengths:
        out.append(off)
        off += n + 1
    return out


class Scenario:
    def __init__(self, shape, seed):
        self.shape, self.pattern = shape, SHAPES[shape]
        self.L = L = len(self.pattern)
        rng = np.random.default_rng(9000 + 100 * list(SHAPES).index(shape) + seed)
        self.names = [n + " test contig" for n, _ in CONTIGS]  # (a chromosome is found by the first word)
        self.chroms = [n for n, _ in CONTIGS]
        seqs = [pc.rnd(rng, n) for _, n in CONTIGS]
        slots = [(c, s) for c, (_, n) in enumerate(CONTIGS) for s in range(n // SLOT)]
        order = rng.permutation(len(slots))
        free = [j for j, ch in enumerate(self.pattern) if ch == "N"]
        # guides: a protospacer at the pattern's N positions, N at its PAM letters
        self.guides = ["".join(pc.rnd(rng, 1) if ch == "N" else "N" for ch in self.pattern) for _ in range(N_GUIDES)]
        self.loci, sites = [], []
        for i, g in enumerate(self.guides):  # the on-targets, alternating strands
            c, s = slots[order[i]]
            pos, strand = s * SLOT + SITE_AT, i & 1
            site = pc.make_site(rng, self.pattern, g)
            seqs[c] = pc.put(seqs[c], pos, pc.rc(site) if strand else site)
            self.loci.append((c, pos, strand))
            sites.append((c, pos))
        for k in range(N_PLANTED + N_EDGE):  # off-targets: 0-4 substitutions in the protospacer, every second one '-'
            c, s = slots[order[N_GUIDES + k]]
            pos = s * SLOT + SITE_AT
            subs = set(int(x) for x in rng.choice(free, size=int(rng.integers(0, 5)), replace=False))
            site = pc.make_site(rng, self.pattern, self.guides[int(rng.integers(0, N_GUIDES))], subs)
            seqs[c] = pc.put(seqs[c], pos, pc.rc(site) if k & 1 else site)
            sites.append((c, pos))
        self.seqs = seqs
        self.genome = dict(zip(self.chroms, seqs))
        self.records = list(zip(self.names, seqs))
        lines = []
        for c, pos in sites[:N_GUIDES + N_PLANTED]:  # 1-4 variants around 75 % of the sites, at least 7 bases apart
            if rng.random() >= 0.75:
                continue
            offs = []
            for _ in range(int(rng.integers(1, 5))):
                o = int(rng.integers(-30, L + 22))
                if all(abs(o - x) >= 7 for x in offs):
                    offs.append(o)
            for o in offs:
                lines.append(self._vcf_line(rng, c, pos + o))
        for c, pos in sites[N_GUIDES + N_PLANTED:]:  # the right-edge sites: one lone heterozygous SNP on the site's first base -
            ref = seqs[c][pos]                        # its REF window [pos - L + 1, pos + L) ends where the site ends
            lines.append("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t0|1\t1|0\n" % (self.chroms[c], pos + 1, ref, "G" if ref != "G" else "T"))
        rng.shuffle(lines)
        self.vcf = vcf_header(2) + "".join(lines)
        # a variant 5 bases into chr2: its window starts before the contig (an unsigned start that wrapped)
        ref = seqs[1][4]
        self.vcf_wrapped = self.vcf + "chr2\t5\t.\t%s\t%s\t.\tPASS\t.\tGT\t1|1\t0|1\n" % (ref, "G" if ref != "G" else "T")
        # a sample without any alt allele
        self.vcf_no_alt = vcf_header(1) + "".join("\t".join(l.split("\t")[:9]) + "\t0|0\n" for l in lines[:20])
        self.table = ptc.random_pattern_table(np.random.default_rng(500 + seed), ptc.shape_of(self.pattern), zeros=L, ones=8)

    def _vcf_line(self, rng, c, p):
        seq = self.seqs[c]
        ref, kind = seq[p], rng.random()

        def other(b):
            return str(rng.choice([x for x in "ACGT" if x != b]))
        if kind < 0.15:
            r, a = seq[p:p + 1 + int(rng.integers(1, 6))], ref
        elif kind < 0.30:
            r, a = ref, ref + pc.rnd(rng, int(rng.integers(1, 5)))
        else:
            r, a = ref, other(ref)
        alts = [a]
        if rng.random() < 0.3:
            second = other(r[0]) + r[1:]
            alts.append(r + pc.rnd(rng, 2) if second == a or rng.random() < 0.5 else second)
        gts = [GENOTYPES[int(rng.integers(0, len(GENOTYPES)))] for _ in range(2)]
        if len(alts) == 1:
            gts = [g.replace("2", "1") for g in gts]
        return "%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t%s\n" % (self.chroms[c], p + 1, r, ",".join(alts), "\t".join(gts))

    @functools.lru_cache(maxsize=None)
    def windows(self, sample=0, which="vcf"):
        """[(id, sequence)] of the sample's window genome for sites of L bases, by the oracle's vcf_loader."""
        return vo.vcf_loader(getattr(self, which), self.genome, sample, self.L)

    @functools.lru_cache(maxsize=None)
    def case(self, m=M, sample=0):
        return Case(self, m, sample)


def empty_rows(n):
    return {"count": np.zeros((n, 9), dtype=np.int64), "on_target": np.zeros(n, dtype=np.int64), "dropped": np.zeros(n, dtype=np.int64),
            "score_sum": np.zeros(n, dtype=np.int64), "positive": np.zeros(n, dtype=np.int64), "positive_nm": np.zeros((n, 9), dtype=np.int64)}


def add_row(rows, g, nm, f):
    rows["count"][g, nm] += 1
    rows["score_sum"][g] += int(f)
    if f:
        rows["positive"][g] += 1
        rows["positive_nm"][g, nm] += 1


def walk(fid, pos, L):
    """(pos2, tag, shifted) of the site of L bases at window position pos of the window with the split id fid."""
    pot = mo.Pot("", fid[0], (pos + mo.c_atoi(fid[1] if len(fid) > 1 else "0")) % (1 << 32), "+", "", [])
    pos1 = pot.pos
    mo.get_snp_type(pot, fid, L)
    return pot.pos, pot.snp_type, pot.pos != pos1


def n_var_of(tag):
    return 0 if tag == "REF" else tag.count(",") + 1


class Case:
    """One (max mismatches, sample) of a scenario, everything from the oracles: both searches in the pattern search's order
    with the mergers' verdict per record, the f word per record, and the expected rows of the screen."""

    def __init__(self, sc, m, sample):
        self.sc, self.m, self.sample = sc, m, sample
        L = sc.L
        self.windows = sc.windows(sample)
        ids, wseqs = [w[0] for w in self.windows], [w[1] for w in self.windows]
        self.info = [w[0].split("_") + [str(len(w[1]))] for w in self.windows]
        # ---- the window side: filterSnpAlignment (merge_oracle.merge_results) over the records in the search's order
        self.win_hits, _ = pc.brute_force(wseqs, sc.pattern, sc.guides, m)
        self.win_rec, _ = pc.arrays(self.win_hits, N_GUIDES)
        self.win_f = ptc.scored(wseqs, sc.guides, self.win_hits, sc.table)
        n = len(self.win_hits)
        self.label = np.zeros(n, dtype=[("chr", "U16"), ("pos", "<u4"), ("n_var", "<u4"), ("var", "?"), ("dup", "?"), ("on", "?")])
        self.shifted, self.right_edge, keys = 0, 0, []
        for i, (g, strand, w, p, nm, mask) in enumerate(self.win_hits):
            fid = ids[w].split("_")
            pos2, tag, moved = walk(fid, p, L)
            self.shifted += moved
            self.right_edge += p + L == len(wseqs[w])
            site = mo.dna5(wseqs[w][p:p + L])
            keys.append((g, fid[0], pos2, strand, pc.rc(site) if strand else site, mask, tag))
            c0, p0, s0 = sc.loci[g]
            on = fid[0] == sc.chroms[c0] and pos2 == p0 and strand == s0 and nm == 0 and tag == "REF"
            self.label[i] = (fid[0], pos2, n_var_of(tag), tag != "REF", i > 0 and keys[i] == keys[i - 1], on)
        self.keys = keys
        # ---- the reference side: filterRefAlignment with seq_len = L
        self.ref_hits, _ = pc.brute_force(sc.seqs, sc.pattern, sc.guides, m)
        self.ref_rec, _ = pc.arrays(self.ref_hits, N_GUIDES)
        self.ref_f = ptc.scored(sc.seqs, sc.guides, self.ref_hits, sc.table)
        self.ref_shadowed = np.array([shadows(self.info, sc.chroms[c], p, L) for _, _, c, p, _, _ in self.ref_hits], dtype=bool)
        self.ref_on = np.array([(c, p, s) == sc.loci[g] and nm == 0 for g, s, c, p, nm, _ in self.ref_hits], dtype=bool)

    def window_offsets(self):
        return plane_offsets([len(w[1]) for w in self.windows])

    @functools.lru_cache(maxsize=None)
    def rows(self, exclude=True):
        """{"ref", "win", "var"}: the rows of the three kinds, count / on_target / dropped and the table fields."""
        ref, win, var = empty_rows(N_GUIDES), empty_rows(N_GUIDES), empty_rows(N_GUIDES)
        for i, (g, _, _, _, nm, _) in enumerate(self.ref_hits):
            on = exclude and self.ref_on[i]
            ref["dropped"][g] += bool(self.ref_shadowed[i])
            if on:
                ref["on_target"][g] = 1
            if not on and not self.ref_shadowed[i]:
                add_row(ref, g, nm, self.ref_f[i])
        for i, (g, _, _, _, nm, _) in enumerate(self.win_hits):
            on = exclude and self.label["on"][i]
            win["dropped"][g] += bool(self.label["dup"][i])
            if on:
                win["on_target"][g] = var["on_target"][g] = 1
            if not on and not self.label["dup"][i]:
                add_row(win, g, nm, self.win_f[i])
                if self.label["var"][i]:
                    add_row(var, g, nm, self.win_f[i])
        return {"ref": ref, "win": win, "var": var}

    def individual(self, exclude=True):
        r = self.rows(exclude)
        return {f: r["ref"][f] + r["win"][f] for f in ("count", "score_sum", "positive", "positive_nm")}

    def floors(self):
        """The categories of FLOORS, counted on the oracle's output."""
        lab, L = self.label, self.sc.L
        counted = ~lab["dup"] & ~lab["on"]
        kept, apart = {}, 0
        for i in np.flatnonzero(counted):
            apart += self.keys[i] in kept and kept[self.keys[i]] != i - 1
            kept[self.keys[i]] = i
        off = self.window_offsets()
        bit = np.array([(off[w] + p) & 31 for _, _, w, p, _, _ in self.win_hits])
        return {"dup_adjacent": int(lab["dup"].sum()), "var_records": int(lab["var"].sum()), "dup_apart": int(apart),
                "multi_var": int((lab["n_var"] >= 2).sum()), "on_target_in_window": int(lab["on"].sum()), "shifted": int(self.shifted),
                "shadowed": int(self.ref_shadowed.sum()), "right_edge": int(self.right_edge), "straddle": int((bit + L > 32).sum()),
                "bit0": int((bit == 0).sum())}


@functools.lru_cache(maxsize=None)
def scenario(shape, seed=None):
    return Scenario(shape, SEEDS[shape] if seed is None else seed)

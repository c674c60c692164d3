"""The scenario of the variant-aware screen (tests/test_variants_map_cpu.py, tests/test_variants_screen.py): a genome small
enough for the Python oracle and dense enough to reach every branch of the mergers' window side - duplicates next to each other
and apart, hits that cover one and several variants, on-targets inside windows, indel shifts, shadowed reference hits, a
chromosome whose name holds '_'.  The oracle side is oracle/variants_oracle.py (the windows), oracle/pyoracle.py (the searches)
and oracle/merge_oracle.py (the merger); nothing here touches the product."""
import functools

import numpy as np

from helpers import mutate, random_seq, revcomp
from oracle import merge_oracle as mo
from oracle import pyoracle
from oracle import variants_oracle as vo

CONTIGS = [("chr1", 24000), ("chr2", 14000), ("chrUn_x", 2500)]
SLOT, SITE_AT = 150, 60  # one site per slot of 150 bases, 60 bases into it: variants at -30 .. +44 (+ a deletion) stay inside
N_GUIDES, N_PLANTED = 24, 240
GENOTYPES = ["0|1", "1|0", "1|1", "0/1", "1/1", "1|2", "2|1", "1/2", "0|2"]
CASES = [(4, 0), (6, 1)]  # (max mismatches, sample column)
SEEDS = [1, 3]
# what every (seed, case) of the scenario must hold, counted on the oracle's own output (Scenario.floors)
FLOORS = {"dup_adjacent": 5, "dup_apart": 1, "var_rows": 40, "multi_var": 5, "on_target": 1, "shifted": 10, "shadowed": 50,
          "chrun_windows": 10}


def vcf_header(n_samples):
    return "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join("S%d" % i for i in range(n_samples)) + "\n"


class Scenario:
    def __init__(self, seed):
        rng = np.random.default_rng(7000 + seed)
        self.names = [n + " test contig" for n, _ in CONTIGS]  # (a chromosome is found by the first word)
        self.chroms = [n for n, _ in CONTIGS]
        seqs = [random_seq(rng, n) for _, n in CONTIGS]
        slots = [(c, s) for c, (_, n) in enumerate(CONTIGS) for s in range(n // SLOT)]
        order = rng.permutation(len(slots))
        self.guides = [random_seq(rng, 21) + "GG" for _ in range(N_GUIDES)]
        self.guide_names = ["g%d" % i for i in range(N_GUIDES)]
        self.loci, sites = [], []
        for i, g in enumerate(self.guides):  # the on-targets, alternating strands
            c, s = slots[order[i]]
            pos, strand = s * SLOT + SITE_AT, i & 1
            seqs[c] = seqs[c][:pos] + (revcomp(g) if strand else g) + seqs[c][pos + 23:]
            self.loci.append((c, pos, strand))
            sites.append((c, pos))
        for k in range(N_PLANTED):  # off-targets: 0-4 substitutions in the protospacer, 30 % with PAM GA, every second one '-'
            c, s = slots[order[N_GUIDES + k]]
            pos = s * SLOT + SITE_AT
            site = mutate(rng, self.guides[int(rng.integers(0, N_GUIDES))], int(rng.integers(0, 5)), 0, 20)
            if rng.random() < 0.3:
                site = site[:21] + "GA"
            seqs[c] = seqs[c][:pos] + (revcomp(site) if k & 1 else site) + seqs[c][pos + 23:]
            sites.append((c, pos))
        self.seqs = seqs
        self.genome = dict(zip(self.chroms, seqs))
        self.records = list(zip(self.names, seqs))
        self.bed = "".join("%s\t%d\t%d\t%s\t0\t%s\n" % (self.chroms[c], p, p + 23, self.guide_names[i], "-" if s else "+")
                           for i, (c, p, s) in enumerate(self.loci))
        lines = []
        for c, pos in sites:  # 1-4 variants around 75 % of the sites, at least 7 bases apart (no deletion reaches the next one)
            if rng.random() >= 0.75:
                continue
            offs = []
            for _ in range(int(rng.integers(1, 5))):
                o = int(rng.integers(-30, 45))
                if all(abs(o - x) >= 7 for x in offs):
                    offs.append(o)
            for o in offs:
                lines.append(self._vcf_line(rng, c, pos + o))
        rng.shuffle(lines)
        self.vcf = vcf_header(2) + "".join(lines)
        # a variant 5 bases into chr2: its window starts before the contig (an unsigned start that wrapped)
        ref = seqs[1][4]
        self.vcf_wrapped = self.vcf + "chr2\t5\t.\t%s\t%s\t.\tPASS\t.\tGT\t1|1\t0|1\n" % (ref, "G" if ref != "G" else "T")
        # a sample without any alt allele
        self.vcf_no_alt = vcf_header(1) + "".join("\t".join(l.split("\t")[:9]) + "\t0|0\n" for l in lines[:20])

    def _vcf_line(self, rng, c, p):
        seq = self.seqs[c]
        ref, kind = seq[p], rng.random()

        def other(b):
            return str(rng.choice([x for x in "ACGT" if x != b]))
        if kind < 0.15:
            r, a = seq[p:p + 1 + int(rng.integers(1, 6))], ref
        elif kind < 0.30:
            r, a = ref, ref + random_seq(rng, int(rng.integers(1, 5)))
        else:
            r, a = ref, other(ref)
        alts = [a]
        if rng.random() < 0.3:
            second = other(r[0]) + r[1:]
            alts.append(r + random_seq(rng, 2) if second == a or rng.random() < 0.5 else second)
        gts = [GENOTYPES[int(rng.integers(0, len(GENOTYPES)))] for _ in range(2)]
        if len(alts) == 1:
            gts = [g.replace("2", "1") for g in gts]
        return "%s\t%d\t.\t%s\t%s\t.\tPASS\t.\tGT\t%s\n" % (self.chroms[c], p + 1, r, ",".join(alts), "\t".join(gts))

    @functools.lru_cache(maxsize=None)
    def windows(self, sample, which="vcf"):
        """[(id, sequence)] of the sample's window genome, by the oracle's vcf_loader."""
        return vo.vcf_loader(getattr(self, which), self.genome, sample, 23)

    @functools.lru_cache(maxsize=None)
    def case(self, m, sample):
        return Case(self, m, sample)


def positions_of(mask):
    return [b for b in range(23) if (mask >> b) & 1] or [-1]


def mit_fixed(positions):
    s, ub = pyoracle.mit_score(positions)
    return int(np.rint(s * 2.0 ** 24)), int(ub)


def empty_rows(n):
    return {"nm": np.zeros((n, 9), dtype=np.int64), "mit_sum": np.zeros(n, dtype=np.int64), "mit_ub": np.zeros(n, dtype=np.int64),
            "on_target": np.zeros(n, dtype=np.int64)}


def add_row(rows, g, positions):
    fixed, ub = mit_fixed(positions)
    rows["nm"][g, 0 if positions == [-1] else len(positions)] += 1
    rows["mit_sum"][g] += fixed
    rows["mit_ub"][g] += ub


class Case:
    """One (max mismatches, sample) of a scenario, everything from the oracle: the window search in vsc_search order with
    the merger's verdict per record, the expected rows of the screen, and the merger's own TSV with its per-guide sums."""

    def __init__(self, sc, m, sample):
        self.sc, self.m, self.sample = sc, m, sample
        self.windows = sc.windows(sample)
        ids, wseqs = [w[0] for w in self.windows], [w[1] for w in self.windows]
        ref = mo.Genome(sc.records)
        on, _ = mo.read_ontargets(sc.bed, ref)
        self.hits = pyoracle.search(wseqs, sc.guides, m, mode=pyoracle.MODE_PREDICATE)  # vsc_search's records and order
        n = len(self.hits)
        self.label = np.zeros(n, dtype=[("chr", "U16"), ("pos", "<u4"), ("n_var", "<u4"), ("var", "?"), ("dup", "?"), ("on", "?")])
        self.shifted = 0
        keys = []
        for i, h in enumerate(self.hits):  # filterSnpAlignment (merge_oracle.merge_results) over the records in that order
            strand = "-" if int(h["info"]) >> 31 else "+"
            w, p = int(h["contig"]), int(h["pos"])
            site = mo.dna5(wseqs[w][p:p + 23])
            fid = ids[w].split("_")
            pot = mo.Pot(sc.guide_names[int(h["guide"])], fid[0], (p + mo.c_atoi(fid[1] if len(fid) > 1 else "0")) % (1 << 32), strand,
                         revcomp(site) if strand == "-" else site, positions_of(int(h["info"]) & 0x7FFFFF))
            pos1 = pot.pos
            mo.get_snp_type(pot, fid, 23)
            self.shifted += pot.pos != pos1
            keys.append(pot.key())
            tag = pot.snp_type
            self.label[i] = (fid[0], pot.pos, 0 if tag == "REF" else tag.count(",") + 1, tag != "REF", i > 0 and keys[i] == keys[i - 1],
                             keys[i] == on[pot.target].key())
        self.keys = keys
        counted = ~self.label["dup"] & ~self.label["on"]
        self.rows_all, self.rows_var = empty_rows(N_GUIDES), empty_rows(N_GUIDES)
        self.dups = np.zeros(N_GUIDES, dtype=np.int64)
        for i, h in enumerate(self.hits):
            g = int(h["guide"])
            self.dups[g] += bool(self.label["dup"][i])
            if self.label["on"][i]:
                self.rows_all["on_target"][g] = self.rows_var["on_target"][g] = 1
            if counted[i]:
                add_row(self.rows_all, g, list(keys[i][5]))
                if self.label["var"][i]:
                    add_row(self.rows_var, g, list(keys[i][5]))
        self.counted = counted

    @functools.cached_property
    def merged(self):
        """The per-guide sums of the TSV mergeResults prints for the two SAM files of the oracle's searches: rows as the
        screen's, and the rows of the reference side alone."""
        sc = self.sc
        ids, wseqs = [w[0] for w in self.windows], [w[1] for w in self.windows]
        ref_sam = pyoracle.search_sam(sc.seqs, sc.chroms, sc.guides, sc.guide_names, self.m)
        snp_sam = in_search_order(pyoracle.search_sam(wseqs, ids, sc.guides, sc.guide_names, self.m), sc.guide_names, ids)
        tsv, _ = mo.merge_results(ref_sam, snp_sam, sc.bed, sc.records, self.windows, "", 23, False)
        rows = empty_rows(N_GUIDES)
        for line in tsv.splitlines()[1:]:
            f = line.split("\t")
            g = sc.guide_names.index(f[3].rsplit("_", 1)[0])
            positions = [int(x) for x in f[8].split(",")] if f[8] else [-1]
            assert int(f[7]) == (0 if positions == [-1] else len(positions))
            add_row(rows, g, positions)
        self.ref_hits = sum(1 for l in ref_sam.splitlines() if l and not l.startswith("@"))
        return rows

    def floors(self):
        """The categories of FLOORS, counted on the oracle's output."""
        lab, kept = self.label, {}
        apart = 0
        for i in np.flatnonzero(self.counted):
            apart += self.keys[i] in kept and kept[self.keys[i]] != i - 1
            kept[self.keys[i]] = i
        sc = self.sc
        info = [w[0].split("_") + [str(len(w[1]))] for w in self.windows]
        ref_hits = pyoracle.search(sc.seqs, sc.guides, self.m, mode=pyoracle.MODE_PREDICATE)
        shadowed = sum(shadows(info, sc.chroms[int(h["contig"])], int(h["pos"])) for h in ref_hits)
        return {"dup_adjacent": int(lab["dup"].sum()), "dup_apart": int(apart), "var_rows": int((lab["var"] & self.counted).sum()),
                "multi_var": int(((lab["n_var"] >= 2) & self.counted).sum()), "on_target": int(lab["on"].sum()), "shifted": int(self.shifted),
                "shadowed": int(shadowed), "chrun_windows": sum(1 for w in self.windows if w[0].startswith("chrUn_x_"))}


def in_search_order(sam, guide_names, contig_names):
    """The records of a SAM text in vsc_search's order (guide, '+' before '-', contig, position).  bidir_mapping writes a block
    in that order except that it holds the best record so far back (bidir_mapping.cpp:167-187); the merger's duplicate rule
    looks at the record before, so its outcome depends on the order, and the screen is defined on vsc_search's."""
    g, c = {n: i for i, n in enumerate(guide_names)}, {n: i for i, n in enumerate(contig_names)}
    head = [l for l in sam.splitlines() if l.startswith("@")]
    rows = [l.split("\t") for l in sam.splitlines() if l and not l.startswith("@")]
    rows.sort(key=lambda f: (g[f[0]], (int(f[1]) >> 4) & 1, c[f[2]], int(f[3])))
    return "\n".join(head + ["\t".join(f) for f in rows]) + "\n"


def shadows(info, chrom, pos, seq_len=23):
    """filterRefAlignment's predicate (merge_oracle.merge_results): is the reference hit inside a window of its chromosome?"""
    for w in info:
        if w[0] != chrom:
            continue
        s, ln = mo.c_atoi(w[1]), mo.c_atoi(w[-1])
        if pos >= (s % (1 << 32)) and (pos + seq_len) % (1 << 32) <= (s + ln) % (1 << 32):
            return True
    return False


@functools.lru_cache(maxsize=None)
def scenario(seed):
    pyoracle.build()
    return Scenario(seed)

"""The wide cohort of the call family's and the VCF checks' tests: a chain of bubbles walked by more haplotypes, of more samples and
in more genotype slots than a wave has lanes, several times over, so that the lane-per-sample loops of the record kernels
(`for (sm = lane; sm < n_samples; sm += 64)`) take a second and a third round and the ballots of the VCF checks more than two
batches.  What the case must reach is stated on the restatement's output alone (tests/test_cohort_inputs.py, no GPU); the GPU
tests put it through their files' own comparisons."""
import numpy as np

import vcf_ref as V
from povu_amd import workloads as W

UNITS = 12        # bubbles of the chain
HAPLOTYPES = 263  # walks drawn: 261 of them a slot each, two a second contig of a slot that has one
SAMPLES = 131     # ploidies 1, 2, 3, 1, 2, 3, ...: 43 * 6 + 1 + 2 = 261 slots
SEED = 77
SEQ_SEED = 5
MAX_LEN = 6       # of W.random_sequences: short segments, so that the restatement stays quick
BARE = (3, 66, 129)       # samples (ploidy 1) whose path has a plain name, no PanSN
TWO_CONTIGS = (69, 100)   # samples past lane 63 with two contigs in slot 1; 69 has that one slot, 100 a second one
SECOND_DIFFERS = {69: (2, 7), 100: (7, 10)}  # the sites (units) a second contig crosses by another allele than the first
CUT_SAMPLE = 126         # its one haplotype ends in the middle of the chain: no call behind it, and a partial reference
CUT_AT = 3 * (UNITS // 2) + 1  # the segment it ends on (the entry of unit UNITS / 2)
REF_LOW = "s1#1#"         # sample 1, slot 1
REF_HIGH = "s130#2#"      # sample 130, the last slot
REF_PARTIAL = "s126#1#"   # the haplotype that is cut
REFS = (REF_LOW, REF_HIGH)


def ploidy(sample: int) -> int:
    return sample % 3 + 1


def wide_names():
    """The names of the 261 slots' paths in sample order, then the second contigs."""
    names = []
    for s in range(SAMPLES):
        if s in BARE:
            names.append(f"bare{s}")
        else:
            names += [f"s{s}#{h}#c" for h in range(1, ploidy(s) + 1)]
    return names + [f"s{s}#1#d" for s in TWO_CONTIGS]


def _other_alleles(ids, units):
    """The walk `ids` (forward or backward) of the chain with another allele at `units`: x -> y -> the skip -> x."""
    have = set(ids.tolist())
    out = []
    for u in range(UNITS):
        a = 3 * u + 1
        c = 0 if a + 1 in have else 1 if a + 2 in have else 2
        if u in units:
            c = (c + 1) % 3
        out += [a] + ([a + 1 + c] if c < 2 else [])
    out.append(3 * UNITS + 1)
    return np.array(out if ids[0] == 1 else out[::-1], dtype=np.uint32)


def wide_chain():
    """(graph, paths).  Every fourth haplotype is written reversed; the second contig of a TWO_CONTIGS sample walks the chain as
    that sample's first contig does but for the sites of SECOND_DIFFERS, which it crosses by another allele."""
    g = W.chain_of_bubbles(UNITS)
    p = W.chain_haplotypes(UNITS, HAPLOTYPES, seed=SEED)
    names = wide_names()
    assert len(names) == HAPLOTYPES
    pieces = []
    for k, name in enumerate(names):
        a, b = int(p.off[k]), int(p.off[k + 1])
        ids, rev = p.ids[a:b], p.rev[a:b]
        if name == REF_PARTIAL + "c":
            at = int(np.flatnonzero(ids == CUT_AT)[0])
            ids, rev = (ids[:at + 1], rev[:at + 1]) if not rev[0] else (ids[at:], rev[at:])  # segments 1 .. CUT_AT either way
        if name.endswith("#d"):
            first = pieces[names.index(name[:-1] + "c")][0]
            ids = _other_alleles(first, SECOND_DIFFERS[int(name[1:name.index("#")])])
            rev = np.full(ids.size, 0 if ids[0] == 1 else 1, dtype=np.uint8)
        pieces.append((ids, rev))
    return g, W._paths(names, pieces)


def wide_sequences(g):
    return W.random_sequences(g, SEQ_SEED, max_len=MAX_LEN)


def wide_gfa_sequences(g):
    """... for a GFA: an S line needs a sequence."""
    return W.random_sequences(g, SEQ_SEED, max_len=MAX_LEN, empty=0.0)


def steps_of(p):
    return [p.steps(k) for k in range(len(p))]


def without_second_contigs(p):
    """The paths without the second contigs of TWO_CONTIGS."""
    keep = [k for k, n in enumerate(p.names) if not n.endswith("#d")]
    return W._paths([p.names[k] for k in keep], [(p.ids[int(p.off[k]):int(p.off[k + 1])], p.rev[int(p.off[k]):int(p.off[k + 1])]) for k in keep])


# ---- what a kernel that stops after ceil(n / 64) rounds of its per-sample loop would give

def restricted(slots, sample_of, n, alts):
    """(ac, an, ns) of a record's slots with those of the samples of index >= n taken as missing."""
    got = [g if sample_of[sl] < n else None for sl, g in enumerate(slots)]
    ac = [sum(1 for g in got if g == a) for a in range(1, alts + 1)]
    return ac, sum(1 for g in got if g is not None), len({sample_of[sl] for sl, g in enumerate(got) if g is not None})


def restricted_differs(slots, sample_of, n, ac, an, ns):
    return restricted(slots, sample_of, n, len(ac)) != (list(ac), an, ns)


def sample_of_slots(names):
    return V.slots_of(names)[2]

"""The inputs of tests/test_gpu_prim.py meet the conditions that make its comparisons mean something (tests/prim_cases.py), on
the restatement alone.  No GPU."""
import pytest

import inversions_ref as I
import oracle_lib as O
import prim_cases as PC
import prim_ref as PR
import vcf_ref as V


def restated(g, seqs, p, prefixes, cap=0, inversions=False):
    names, paths = list(p.names), [p.steps(i) for i in range(len(p))]
    sq = dict(zip(g.vid.tolist(), seqs))
    sites = V.sites_of_pvst(list(O.decompose(g).values()))
    raw = V.call(sites, names, paths, sq, prefixes)
    if inversions:
        raw = I.merge(raw, I.records(names, paths, sq, prefixes)[0])
    return raw, PR.decompose(raw, names, paths, sq, max_allele_length=cap)


def test_chain_case():
    case = PC.chain_case()
    raw, (rows, counters) = restated(*case, PC.CHAIN_REFS)
    _, (rows_inv, _) = restated(*case, ["hap0"], inversions=True)
    PC.chain_coverage(rows, raw, rows_inv)
    PC.coverage(rows_inv)
    assert counters["n_prim_tier2"] >= 10 and counters["n_prim_cells"] > 513 * 512


@pytest.mark.parametrize("seed", PC.COMPLEX_SEEDS)
def test_complex_case(seed):
    raw, (rows, counters) = restated(*PC.complex_case(seed), ["hap0"], cap=PC.COMPLEX_CAP)
    PC.coverage(rows)
    assert counters["n_decomposed_alts"] > 100 and counters["n_passthrough_alts"] > 20

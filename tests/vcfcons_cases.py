"""Inputs of the consensus haplotypes' tests (tests/test_vcfcons_ref.py, tests/test_gpu_vcfcons.py): the drop rule's cases, the
golden files against their GFAs, and the library's result as the plain lists and texts the restatement (tests/vcfcons_ref.py)
gives."""
import json
import os

import vcf_ref as V
import vcfcmp_ref as M
import vcfcons_ref as CR
import vcfhap_cases as K
import vcfhap_ref as HR

ROOT, GOLDEN, HEAD, vcf, golden, bases, other = K.ROOT, K.GOLDEN, K.HEAD, K.vcf, K.golden, K.bases, K.other
EXPECTED = os.path.join(ROOT, "tests", "golden", "vcfcons_expected.json")
ARRAYS = ("hap_chrom", "hap_col", "hap_phase", "hap_len", "hap_off") + CR.COUNTS + ("rt_status", "rt_path", "rt_path_len", "rt_first_diff")
COUNTERS = ("n_haps", "n_text_bytes", "n_unplaced")
KEY = dict(hap_chrom="chrom", hap_col="col", hap_phase="phase", hap_len="len", hap_off="off")

# ---- the drop rule, case by case: one sample, every GT 1, on the path `c`
PATH_C = "ACGTACGTACGTACGTACGTACGT"
SPAN = ("c", 3, "span", "GTACGT", "CCC")  # replaces [2, 8) by CCC
DROP_CASES = {
    "a parent over two children": [SPAN, ("c", 4, "k1", "T", "A"), ("c", 6, "k2", "C", "G")],
    "a parent equal to a child": [("c", 3, "par", "GTA", "GCA"), ("c", 4, "kid", "T", "C")],
    "an insertion at a span's start": [SPAN, ("c", 2, "ins", "C", "CTT")],
    "an insertion at a span's end": [SPAN, ("c", 8, "ins", "T", "TGG")],
    "an insertion inside a span": [SPAN, ("c", 5, "ins", "A", "AGG")],
    "two insertions at one point": [("c", 2, "i1", "C", "CTT"), ("c", 2, "i2", "C", "CGG")],
    "the chain A B C": [("c", 1, "A", PATH_C[0:10], "TTG"), ("c", 6, "B", PATH_C[5:20], "AA"), ("c", 13, "C", PATH_C[12:15], "TT")],
}
# (applied, duplicate, enclosed, overlap) and the text, worked by hand from the definition
DROP_PINS = {
    "a parent over two children": ((1, 0, 2, 0), "ACCCCACGTACGTACGTACGT"),
    "a parent equal to a child": ((1, 1, 0, 0), "ACGCACGTACGTACGTACGTACGT"),
    "an insertion at a span's start": ((2, 0, 0, 0), "ACTTCCCACGTACGTACGTACGT"),
    "an insertion at a span's end": ((2, 0, 0, 0), "ACCCCGGACGTACGTACGTACGT"),
    "an insertion inside a span": ((1, 0, 1, 0), "ACCCCACGTACGTACGTACGT"),
    "two insertions at one point": ((1, 0, 0, 1), "ACTTGTACGTACGTACGTACGTACGT"),
    "the chain A B C": ((1, 0, 1, 1), "TTGGTACGTACGTACGT"),
}


def drop_case(name: str):
    """(VCF text, [(path name, bases)]) of a drop case."""
    return vcf(["s"], [row + (["1"],) for row in DROP_CASES[name]]), [("c", PATH_C)]


def gfa_named(fixture_path: str):
    """(path names, {name: bases}) of a GFA."""
    names, paths, seqs = V.read_gfa(fixture_path)
    return list(names), HR.path_bases(names, paths, seqs)


def ref_run(text: str, names, ref: dict, roundtrip=True, samples=None, chroms=None, force=False) -> dict:
    """The restatement on VCF text; samples / chroms: names, as HipDecomposer.consensus takes them."""
    doc = M.parse(text)
    cols = None if samples is None else {c for c, n in enumerate(doc["samples"]) if n in samples}
    ids = None if chroms is None else {doc["chroms"].index(x) for x in chroms}
    return CR.consensus(doc, list(names), ref, roundtrip, cols, ids, force), doc


def ref_digest(res: dict, doc: dict, names) -> dict:
    out = {k: [h[KEY.get(k, k)] for h in res["haps"]] for k in ARRAYS}
    out.update({k: res[k] for k in COUNTERS})
    out.update(texts=[h["text"] for h in res["haps"]], fasta=CR.fasta_text(doc, res), roundtrip=CR.roundtrip_text(doc, res, names),
               summary=CR.summary_text(res))
    return out


def lib_digest(c) -> dict:
    out = {k: getattr(c, k).tolist() for k in ARRAYS}
    out.update({k: getattr(c, k) for k in COUNTERS})
    out.update(texts=[c.sequence(i) for i in range(c.n_haps)], fasta=c.fasta_text(), roundtrip=c.roundtrip_text(), summary=c.summary_text())
    return out


def both_tiers(d, text: str, names, ref: dict, roundtrip=True, samples=None, chroms=None):
    """The consensus of `text` on the paths resident in `d` with and without the forced second tier: each equals the
    restatement array for array and text for text, n_tier2 is the restatement's; returns (the first result, the restatement's)."""
    first = None
    for force in (False, True):
        want, doc = ref_run(text, names, ref, roundtrip, samples, chroms, force)
        got = d.consensus(text, roundtrip=roundtrip, samples=samples, chroms=chroms, force_tier2=force)
        have, wanted = lib_digest(got), ref_digest(want, doc, names)
        for k in wanted:
            assert have[k] == wanted[k], (k, force, have[k], wanted[k])
        assert got.n_tier2 == want["n_tier2"] and got.roundtrip == roundtrip, force
        for width in (0, 1, 7):
            assert got.fasta_text(width) == CR.fasta_text(doc, want, width), width
        if first is None:
            first = (got, want)
    assert lib_digest(got) == lib_digest(first[0])  # the two tiers, against each other: equal but for n_tier2
    return first


def statuses(res: dict):
    return [CR.RT_NAME[h["rt_status"]] for h in res["haps"]]


def expected() -> dict:
    return json.load(open(EXPECTED))


def expected_now() -> dict:
    """What tests/golden/vcfcons_expected.json holds: the restatement's digest of every drop case."""
    out = {}
    for name in DROP_CASES:
        text, named = drop_case(name)
        res, doc = ref_run(text, [n for n, _ in named], dict(named))
        out[name] = ref_digest(res, doc, [n for n, _ in named])
    return out


def write_expected() -> None:
    with open(EXPECTED, "w") as f:
        json.dump(expected_now(), f, indent=1, sort_keys=True)
        f.write("\n")


def upload_gfa_file(d, gfa: str):
    """Makes a GFA resident in `d` (graph, paths, sequences); returns (path names, {name: bases})."""
    import numpy as np
    from povu_amd import workloads as W
    names, paths, seqs = V.read_gfa(gfa)
    ids = sorted(seqs)
    at = {v: k for k, v in enumerate(ids)}
    links = [ln.rstrip("\n").split("\t") for ln in open(gfa) if ln.startswith("L\t")]
    side = lambda o, plus: [plus if f == "+" else W.L + W.R - plus for f in o]  # noqa: E731
    g = W._mk(np.array(ids), np.array([at[int(f[1])] for f in links]), np.array(side([f[2] for f in links], W.R)),
              np.array([at[int(f[3])] for f in links]), np.array(side([f[4] for f in links], W.L)))
    d.upload(g)
    d.upload_paths(W._paths(names, [([i for i, _ in st], [r for _, r in st]) for st in paths]))
    d.upload_sequences([seqs[i] for i in ids])
    return list(names), HR.path_bases(names, paths, seqs)


def upload_named(d, named):
    """Makes paths that spell the given bases resident in `d` (vcfhap_cases.reference_graph: chains of short segments, every
    third walked backwards); returns (path names, {name: bases})."""
    K.upload_reference(d, named)
    return [n for n, _ in named], dict(named)

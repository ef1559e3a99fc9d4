"""Inputs of the haplotype comparison's tests (tests/test_vcfhap_ref.py, tests/test_gpu_vcfhap.py, tests/test_vcfhap_cli.py): the
golden pairs in both modes, a graph whose paths spell given bases, and the library's result as the plain lists and texts the
restatement (tests/vcfhap_ref.py) gives."""
import json
import os

import numpy as np

import vcf_ref as V
import vcfcmp_cases as K
import vcfcmp_ref as M
import vcfhap_ref as HR

ROOT, GOLDEN, HEAD, vcf, golden, bases, other = K.ROOT, K.GOLDEN, K.HEAD, K.vcf, K.golden, K.bases, K.other
GFA_DIR = os.path.join(ROOT, "tests", "golden", "gfa", "downstream_repetitive")
EXPECTED = os.path.join(ROOT, "tests", "golden", "vcfhap_expected.json")
REC_ARRAYS = ("rec_placed", "rec_window")
ITEM_ARRAYS = ("item_record", "item_alt", "item_state", "item_s", "item_e", "item_suffix", "item_prefix", "item_left", "item_right", "item_group")
WIN_ARRAYS = ("win_chrom", "win_lo", "win_hi", "win_n_a", "win_n_b", "win_inconsistent", "win_offender")
CELL_ARRAYS = ("cell_window", "cell_sample", "cell_phase", "cell_status", "cell_edits_a", "cell_edits_b", "cell_len_a", "cell_len_b", "cell_first_diff")
COUNTERS = ("n_records_a", "n_records_b", "n_items_a", "n_items_b", "n_groups", "n_windows", "n_cells", "n_common_samples", "n_inconsistent",
            "n_unplaced_a", "n_unplaced_b", "n_reach_capped")


def gfa_path(fixture: str) -> str:
    return os.path.join(GFA_DIR, fixture + ".gfa")


def gfa_reference(fixture: str) -> dict:
    """The bases of every path of a fixture's GFA by name."""
    return HR.path_bases(*V.read_gfa(gfa_path(fixture)))


def golden_pairs():
    """(fixture, A, B, reference mode) for every golden pair, raw against every profile, in both modes."""
    return [(fx, names[0], name, ref) for fx, names in sorted(K.GOLDEN_FILES.items()) for name in names[1:] for ref in (False, True)]


def pair_key(fixture, a, b, ref) -> str:
    return f"{fixture}:{a}:{b}:{'reference' if ref else 'ref-fields'}"


def ref_arrays(res: dict) -> dict:
    """The restatement's result as the arrays of povu_hip_vcf_hap."""
    key = dict(item_record="record", item_alt="alt", item_state="state", item_s="s", item_e="e", item_suffix="suffix", item_prefix="prefix",
               item_left="left", item_right="right", item_group="group")
    out = {}
    for side in "ab":
        out[f"rec_placed_{side}"] = [int(r["placed"]) for r in res[f"recs_{side}"]]
        out[f"rec_window_{side}"] = [r["window"] for r in res[f"recs_{side}"]]
        for k in ITEM_ARRAYS:
            out[f"{k}_{side}"] = [it[key[k]] for it in res[f"items_{side}"]]
    wkey = dict(win_chrom="chrom", win_lo="lo", win_hi="hi", win_n_a="n_a", win_n_b="n_b", win_inconsistent="inconsistent", win_offender="offender")
    for k in WIN_ARRAYS:
        out[k] = [w[wkey[k]] for w in res["windows"]]
    for k in CELL_ARRAYS:
        out[k] = [c[k[5:]] for c in res["cells"]]
    out["sample_col_a"] = [s["col_a"] for s in res["samples"]]
    out["sample_col_b"] = [s["col_b"] for s in res["samples"]]
    out["sample_status"] = [list(s["counts"]) for s in res["samples"]]
    out["n_status"] = list(res["n_status"])
    out.update({k: res[k] for k in COUNTERS})
    return out


def lib_arrays(h) -> dict:
    """A HapComparison likewise (n_tier2, n_splits and device_ms apart)."""
    out = {}
    for side in "ab":
        for k in REC_ARRAYS + ITEM_ARRAYS:
            out[f"{k}_{side}"] = getattr(h, f"{k}_{side}").tolist()
    for k in WIN_ARRAYS + CELL_ARRAYS + ("sample_col_a", "sample_col_b", "sample_status"):
        out[k] = getattr(h, k).tolist()
    out["n_status"] = list(h.n_status)
    out.update({k: getattr(h, k) for k in COUNTERS})
    return out


def digest(h) -> dict:
    return dict(lib_arrays(h), haplotypes=h.haplotypes_text(), summary=h.summary_text())


def ref_digest(res: dict) -> dict:
    return dict(ref_arrays(res), haplotypes=HR.haplotypes_text(res), summary=HR.summary_text(res))


def expected() -> dict:
    return json.load(open(EXPECTED))


def write_expected() -> None:
    """tests/golden/vcfhap_expected.json: the restatement's digest of every golden pair in both modes."""
    out = {}
    for fx, a, b, ref in golden_pairs():
        res = HR.compare(M.parse(golden(fx, a)), M.parse(golden(fx, b)), gfa_reference(fx) if ref else None)
        out[pair_key(fx, a, b, ref)] = ref_digest(res)
    with open(EXPECTED, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def both_tiers(d, a: str, b: str, reference=None, max_reach: int = HR.MAX_REACH_DEFAULT):
    """The haplotype comparison of texts a and b with and without the forced second tier: each equals the restatement array for
    array and text for text, n_tier2 is the restatement's; returns (the first comparison, the restatement's result).
    reference: the bases of the paths resident in `d` by name, or None for the REF-field mode."""
    da, db = M.parse(a), M.parse(b)
    first = None
    for force in (False, True):
        want = HR.compare(da, db, reference, max_reach, force_tier2=force)
        got = d.compare_haplotypes(a, b, reference=reference is not None, max_reach=max_reach, force_tier2=force)
        have, wanted = lib_arrays(got), ref_arrays(want)
        for k in wanted:
            assert have[k] == wanted[k], (k, force, have[k], wanted[k])
        assert got.n_tier2 == want["n_tier2"], force
        assert got.chroms == want["chroms"] and got.reference == (reference is not None)
        assert got.haplotypes_text() == HR.haplotypes_text(want)
        assert got.summary_text() == HR.summary_text(want)
        if first is None:
            first = (got, want)
    assert digest(got) == digest(first[0])  # the two tiers, against each other: equal but for n_tier2
    return first


def revcomp(t: str) -> str:
    return t.translate(str.maketrans("ACGTNacgtn", "TGCANtgcan"))[::-1]


def reference_graph(named):
    """A graph whose paths spell the given bases: named = [(path name, bases)].  Every path is a chain of its own segments of 1 to
    5 bases, every third one walked backwards.  Returns (links, paths, {segment id: sequence})."""
    from povu_amd import workloads as W
    seqs, pieces, v1, s1, v2, s2 = {}, [], [], [], [], []
    nid = 1
    for k, (_, text) in enumerate(named):
        ids, rev, at, n = [], [], 0, 0
        while at < len(text):
            ln = 1 + (n * 7 + k) % 5
            piece, rv = text[at:at + ln], n % 3 == 1
            seqs[nid] = revcomp(piece) if rv else piece
            if ids:
                v1.append(ids[-1] - 1), s1.append(W.L if rev[-1] else W.R), v2.append(nid - 1), s2.append(W.R if rv else W.L)
            ids.append(nid), rev.append(int(rv))
            nid, at, n = nid + 1, at + ln, n + 1
        pieces.append((ids, rev))
    if not seqs:  # (a graph needs a segment)
        seqs[nid] = "N"
    links = W._mk(np.array(sorted(seqs)), np.array(v1, dtype=np.int64), np.array(s1, dtype=np.int64), np.array(v2, dtype=np.int64),
                  np.array(s2, dtype=np.int64))
    return links, W._paths([n for n, _ in named], pieces), seqs


def upload_reference(d, named) -> dict:
    """Makes the paths of reference_graph(named) and their sequences resident in `d`; returns {name: bases}."""
    links, paths, seqs = reference_graph(named)
    d.upload(links)
    d.upload_paths(paths)
    d.upload_sequences(seqs)
    return dict(named)


def upload_gfa(d, fixture: str) -> dict:
    """Makes a fixture's GFA resident in `d` (graph, paths, sequences); returns {path name: bases}."""
    from povu_amd import workloads as W
    gfa = gfa_path(fixture)
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
    return HR.path_bases(names, paths, seqs)

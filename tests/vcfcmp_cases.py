"""Inputs of the VCF comparison's tests (tests/test_vcfcmp_ref.py, tests/test_gpu_vcfcmp.py, tests/test_vcfcmp_cli.py): VCF text
from rows, the golden VCFs, and the library's result as the plain lists and texts the restatement (tests/vcfcmp_ref.py) gives."""
import os

import vcfcmp_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vcf", "downstream_repetitive")
GOLDEN_FILES = {
    "popped-parent-child-rescue": ("raw_graph", "popped", "top_level_only"),
    "subr-inversion-preservation": ("raw_graph", "decomposed_passthrough"),
    "tandem-repeat-left-normalization": ("raw_graph", "left_normalized"),
    "vcfwave-complex-decomposition": ("raw_graph", "decomposed"),
}
COLUMNS = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
HEAD = "##fileformat=VCFv4.2\n" + COLUMNS + "\tFORMAT\t"
ITEM_ARRAYS = ("item_record", "item_alt", "item_state", "item_pos", "item_suffix", "item_prefix", "item_group")
COUNTERS = ("n_shared", "n_only_a", "n_only_b", "n_skipped_a", "n_skipped_b", "n_items_a", "n_items_b", "n_common_samples", "n_samples_only_a",
            "n_samples_only_b")


def golden(fixture: str, name: str) -> str:
    return open(os.path.join(GOLDEN, fixture, name + ".vcf")).read()


def vcf(samples, rows) -> str:
    """rows: (chrom, pos, id, ref, alt, one GT per sample); without samples the eight fixed columns only."""
    if not samples:
        return "##fileformat=VCFv4.2\n" + COLUMNS + "\n" + "".join("\t".join([c, str(p), i, r, a, "60", "PASS", "."]) + "\n" for c, p, i, r, a, _ in rows)
    return HEAD + "\t".join(samples) + "\n" + "".join(
        "\t".join([c, str(p), i, r, a, "60", "PASS", ".", "GT"] + list(g)) + "\n" for c, p, i, r, a, g in rows)


def bases(rng, n: int) -> str:
    return "".join(rng.choice(list("ACGT"), size=n))


def other(base: str) -> str:
    """Another base than `base`, whatever its case."""
    return "C" if base.upper() != "C" else "G"


def ref_arrays(res: dict) -> dict:
    """The restatement's result as the arrays of povu_hip_vcf_cmp."""
    key = dict(item_record="record", item_alt="alt", item_state="state", item_pos="pos", item_suffix="suffix", item_prefix="prefix", item_group="group")
    out = {f"{k}_{side}": [it[key[k]] for it in res[f"items_{side}"]] for k in ITEM_ARRAYS for side in "ab"}
    out.update(group_class=[g["cls"] for g in res["groups"]], group_n_a=[g["n_a"] for g in res["groups"]],
               group_n_b=[g["n_b"] for g in res["groups"]], group_first=[g["first"] for g in res["groups"]])
    for k in ("col_a", "col_b", "tp", "fp", "fn", "gteq"):
        out["sample_" + k] = [int(s[k]) for s in res["samples"]]
    out.update({k: res[k] for k in COUNTERS})
    out["n_groups"] = len(res["groups"])
    return out


def lib_arrays(c) -> dict:
    """A VcfComparison likewise (n_tier2, n_splits and device_ms apart)."""
    out = {f"{k}_{side}": getattr(c, f"{k}_{side}").tolist() for k in ITEM_ARRAYS for side in "ab"}
    for k in ("group_class", "group_n_a", "group_n_b", "group_first", "sample_col_a", "sample_col_b", "sample_tp", "sample_fp", "sample_fn",
              "sample_gteq"):
        out[k] = getattr(c, k).tolist()
    out.update({k: getattr(c, k) for k in COUNTERS + ("n_groups",)})
    return out


def both_tiers(d, a: str, b: str):
    """The comparison of texts a and b with and without the forced second tier: each equals the restatement array for array
    and text for text, n_tier2 is the restatement's; returns (the first comparison, the restatement's result)."""
    da, db = M.parse(a), M.parse(b)
    first = None
    for force in (False, True):
        want = M.compare(da, db, force_tier2=force)
        got = d.compare_vcfs(a, b, force_tier2=force)
        assert got.doc_a.chroms == da["chroms"] and got.doc_b.chroms == db["chroms"]
        have, wanted = lib_arrays(got), ref_arrays(want)
        for k in wanted:
            assert have[k] == wanted[k], (k, force)
        assert got.n_tier2 == want["n_tier2"], force
        assert got.compare_text() == M.compare_text(da, db, want)
        assert got.summary_text() == M.summary_text(want)
        if first is None:
            first = (got, want)
    assert digest(got) == digest(first[0])  # the two tiers, against each other: equal but for n_tier2
    return first


def digest(c) -> dict:
    return dict(lib_arrays(c), compare=c.compare_text(), summary=c.summary_text())

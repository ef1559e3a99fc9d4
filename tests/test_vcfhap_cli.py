"""`povu vcf --compare --haplotypes` (INTEGRATION.md "Haplotype comparison"): haplotypes.tsv and hap_summary.txt equal the
library's texts and the restatement's (tests/vcfhap_ref.py) with and without -i, compare.tsv and summary.txt stay what they
were; the flags that do not go together are refused by name; the text writer on a hand-made result through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vcfcmp_ref as M
import vcfhap_cases as K
import vcfhap_ref as HR
from povu_amd import hip as H

POVU = os.path.join(K.ROOT, "povu_amd", "bin", "povu")
FILES = ("compare.tsv", "summary.txt")
HAP_FILES = ("haplotypes.tsv", "hap_summary.txt")


def _run(*args):
    return subprocess.run([POVU] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


@pytest.mark.gpu
def test_the_four_files_with_and_without_a_gfa(tmp_path):
    fx = "tandem-repeat-left-normalization"
    a, b = os.path.join(K.GOLDEN, fx, "raw_graph.vcf"), os.path.join(K.GOLDEN, fx, "left_normalized.vcf")
    da, db = M.parse(open(a).read()), M.parse(open(b).read())
    plain = tmp_path / "plain"
    r = _run("vcf", "-c", a, "-d", b, "--compare", "-o", plain)
    assert r.returncode == 0 and sorted(os.listdir(plain)) == sorted(FILES), r.stderr
    for extra, ref in (([], None), (["-i", K.gfa_path(fx)], K.gfa_reference(fx)), (["-i", K.gfa_path(fx), "--max-reach=0"], K.gfa_reference(fx))):
        want = HR.compare(da, db, ref, max_reach=0 if "--max-reach=0" in extra else 256)
        out = tmp_path / f"out{len(extra)}"
        r = _run("-t", "2", "vcf", "-c", a, "-d", b, "--compare", "--haplotypes", "-o", out, *extra)  # differences found: still 0
        assert r.returncode == 0, r.stderr
        assert sorted(os.listdir(out)) == sorted(FILES + HAP_FILES)
        assert [(out / f).read_text() for f in HAP_FILES] == [HR.haplotypes_text(want), HR.summary_text(want)]
        assert [(out / f).read_bytes() for f in FILES] == [(plain / f).read_bytes() for f in FILES]  # byte for byte what they were
    assert want["n_windows"] == 2 and want["n_reach_capped"] == 4  # (max reach 0: the two representations fall apart again)
    # without the flag -i stays unread; a GFA that cannot be read with it
    r = _run("vcf", "-i", tmp_path / "nothing.gfa", "-c", a, "-d", b, "--compare", "-o", tmp_path / "again")
    assert r.returncode == 0 and sorted(os.listdir(tmp_path / "again")) == sorted(FILES)
    r = _run("vcf", "-i", tmp_path / "nothing.gfa", "-c", a, "-d", b, "--compare", "--haplotypes", "-o", tmp_path / "no")
    assert r.returncode == 1 and "nothing.gfa" in r.stderr and not (tmp_path / "no" / "haplotypes.tsv").exists()


def test_flags_that_do_not_go_together_are_refused_by_name(tmp_path):
    vcf = tmp_path / "v.vcf"
    vcf.write_text(K.K.COLUMNS + "\n")
    gfa = tmp_path / "g.gfa"
    gfa.write_text("S\t1\tA\n")
    r = _run("vcf", "-i", gfa, "-c", vcf, "--report", "--haplotypes")
    assert r.returncode == 1 and "--haplotypes belongs to --compare, not to --report" in r.stderr
    r = _run("vcf", "-i", gfa, "-c", vcf, "--report", "--max-reach", "5")
    assert r.returncode == 1 and "--max-reach belongs to --compare, not to --report" in r.stderr
    r = _run("vcf", "-i", gfa, "-c", vcf, "-d", vcf, "--compare", "--report", "--haplotypes")
    assert r.returncode == 1 and "--haplotypes" in r.stderr and "--report" in r.stderr
    r = _run("vcf", "-i", gfa, "-c", vcf, "--haplotypes")
    assert r.returncode == 1 and "--haplotypes is read by --compare only" in r.stderr
    r = _run("vcf", "-i", gfa, "-c", vcf, "--max-reach=5")
    assert r.returncode == 1 and "--max-reach is read by --compare only" in r.stderr
    r = _run("vcf", "-c", vcf, "-d", vcf, "--compare", "--max-reach=5")
    assert r.returncode == 1 and "--max-reach is read by --haplotypes only" in r.stderr
    for bad in ("65537", "-1", "many", ""):
        r = _run("vcf", "-c", vcf, "-d", vcf, "--compare", "--haplotypes", "--max-reach=" + bad)
        assert r.returncode == 1 and "'--max-reach' expects a number of bases between 0 and 65536" in r.stderr, bad
    r = _run("vcf", "-c", vcf, "-d", vcf, "--compare", "--haplotypes", "--max-reach")
    assert r.returncode == 1 and "requires an argument" in r.stderr
    help_text = _run("--help").stdout
    assert "--haplotypes" in help_text and "--max-reach" in help_text


def _hand_made(res: dict):
    """A povu_hip_vcf_hap filled by hand from the restatement's result; returns (the struct, what keeps its arrays alive)."""
    arrays = K.ref_arrays(res)
    h, keep = H._VcfHap(), []
    types = {name: t for name, t in H._VcfHap._fields_}
    for name, value in arrays.items():
        t = types.get(name)
        if t is None or not isinstance(value, list) or name == "n_status":
            continue
        ct = t._type_
        arr = np.ascontiguousarray(np.array(value, dtype=np.dtype(ct)).reshape(-1))
        keep.append(arr)
        setattr(h, name, arr.ctypes.data_as(t) if arr.size else t())
    for k in ("n_records_a", "n_records_b", "n_items_a", "n_items_b", "n_groups", "n_windows", "n_cells", "n_common_samples", "n_inconsistent",
              "n_unplaced_a", "n_unplaced_b", "n_reach_capped"):
        setattr(h, k, res[k])
    for k in range(10):
        h.n_status[k] = res["n_status"][k]
    return h, keep


def test_the_text_writer_on_a_hand_made_result():
    lib = H.load_lib()
    a = K.vcf(["s0", "s1", "x"], [("c", 10, "r0", "ACG", "A,ATT,*", ["0", "1|2", "1"]), ("c", 11, "r1", "C", "T", ["1", "3", "0"]),
                                 ("d", 50, "bad", "GG", "G", ["0|1", "0", "0"]), ("c", 5, "u", ".", "G", ["1", "1", "1"])])
    b = K.vcf(["s1", "s0"], [("c", 10, "q0", "ACG", "A", ["1", "0"]), ("d", 50, "bad", "GT", "G", ["0", "0"]), ("e", 7, "late", "A", "AC", ["1|1", "."])])
    da, db = M.parse(a), M.parse(b)
    res = HR.compare(da, db)
    assert res["n_inconsistent"] == 1 and res["n_unplaced_a"] == 1 and len(HR.haplotypes_text(res).split("\n")) > 4
    doc_a, doc_b = H.parse_vcf(a), H.parse_vcf(b)
    h, keep = _hand_made(res)

    def texts(hp):
        ln, sl, sp = C.c_size_t(0), C.c_size_t(0), C.c_void_p(None)
        p = lib.povu_hip_vcf_hap_text(hp, doc_a._p, doc_b._p, C.byref(ln), C.byref(sp), C.byref(sl))
        if not p:
            return None
        out = C.string_at(p, ln.value).decode(), C.string_at(sp.value, sl.value).decode()
        lib.povu_hip_buffer_free(p)
        lib.povu_hip_buffer_free(sp)
        return out

    assert texts(C.byref(h)) == (HR.haplotypes_text(res), HR.summary_text(res))
    h.n_reach_capped = 3
    assert texts(C.byref(h))[1].endswith("Unplaced records: A 1, B 0\nCapped reaches: 3\n")
    # what does not belong together gives no text: a status, a window, a sample beyond their ranges; null arguments
    for name, value in (("cell_status", 10), ("cell_window", res["n_windows"]), ("cell_sample", res["n_common_samples"]), ("win_chrom", 3)):
        broken, keep2 = _hand_made(res)
        getattr(broken, name)[0] = value
        assert texts(C.byref(broken)) is None, name
    assert texts(None) is None
    empty = HR.compare(M.parse(K.HEAD + "s\n"), M.parse(K.HEAD + "t\n"))
    none = H.parse_vcf(K.HEAD + "s\n")
    doc_a = doc_b = none
    h0, _ = _hand_made(empty)
    assert texts(C.byref(h0)) == (HR.haplotypes_text(empty), HR.summary_text(empty))
    assert texts(C.byref(h0))[1].startswith("Windows: 0, inconsistent 0\n") and "Concordance: nan\nNon-reference concordance: nan\n" in texts(C.byref(h0))[1]

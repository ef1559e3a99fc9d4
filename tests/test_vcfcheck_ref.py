"""The VCF checks without a GPU (INTEGRATION.md "VCF checks"): the restatement (tests/vcfcheck_ref.py), the library's reader
(povu_hip_vcf_parse) and its report text (povu_hip_vcf_report_text) on the reference's nine downstream_repetitive VCF fixtures
against the statuses worked out for them (tests/golden/vcfcheck_expected.json); the reader's refusals and the genotype forms; and
`vcfcheck_check` (povu_amd/csrc/host/vcfcheck_check.cpp, built with -fsanitize=address,undefined): the walk tokenizer and the
occurrence rule the device runs (povu_amd/csrc/hip/vcfcheck_rules.hpp) and the reader, against the restatement."""
import os
import random
import subprocess

import pytest

import vcf_ref as V
import vcfcheck_cases as K
import vcfcheck_ref as R
from povu_amd import hip as H

ROOT = K.ROOT
HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\n"


def vcf(*records, head=HEAD):
    return head + "".join("\t".join(r) + "\n" for r in records)


def rec(info="AT=>1>2>4,>1>3>4", fmt="GT", a="0|1", b="1", pos="5", ref="C", alt="G", ident="x"):
    return ["chr", pos, ident, ref, alt, ".", ".", info, fmt, a, b]


# ---- the nine fixtures

@pytest.mark.parametrize("name", K.FIXTURES)
def test_fixture_statuses(name):
    text, gfa = K.fixture(name)
    want = K.expected()[name]
    names, paths, seqs = V.read_gfa(gfa)
    doc = R.parse(text)
    res = R.check(doc, names, paths, seqs.keys())
    assert K.status_summary(doc, res) == {k: want[k] for k in ("n_records", "n_tasks", "n_status", "failing")}
    assert R.report_text(doc, res, names) == want["report"] and R.summary_text(doc, res) == want["summary"]
    # the library's reader gives the restatement's document, on one thread and on several
    for threads in (1, 4):
        d = H.parse_vcf(text, threads)
        assert K.lib_arrays(d) == R.doc_arrays(doc)
    assert K.lib_texts(d, res, names) == (want["report"], want["summary"])
    # the reference's literal rule finds the same here: no fixture spells a walk backwards
    assert R.check(doc, names, paths, seqs.keys(), forward_only=True)["task_status"] == res["task_status"]


def test_what_the_issue_states_of_the_fixtures():
    exp = K.expected()
    clean = [f for f in K.FIXTURES if f.startswith(("subr-", "vcfwave-")) or f.endswith("/popped.vcf")]
    assert len(clean) == 5 and all(exp[f]["failing"] == [] and exp[f]["n_status"][0] == exp[f]["n_tasks"] for f in clean)
    for f in set(K.FIXTURES) - set(clean):
        assert exp[f]["failing"] == [dict(record=0, allele=0, sample="HG3", phase=0, status="absent")], f
        assert exp[f]["report"].splitlines()[1].split("\t")[4:] == ["1", "HG3", "absent"]
        assert exp[f]["summary"] == "Error rate: %.2f%%\n" % (100 / exp[f]["n_records"])


# ---- the reader

def test_genotype_forms_and_format_position():
    text = vcf(rec(a="0/1", b="."), rec(a="./1", b="1|.|0"), rec(fmt="DP:GT:GQ", a="7:1|0:3", b="9"), rec(fmt="DP", a="3", b="4"),
               ["chr", "9", "y", "A", ".", ".", ".", "AT=>1"], rec(info="NS=2", alt="G,T", a="2", b="5"),
               rec(info="AT=>1,,>2,>7<8", alt="G", a="1", b="3"))
    doc = R.parse(text)
    assert [r["tasks"] for r in doc["records"]] == [[(0, 0, 0), (1, 0, 1)], [(0, 1, 2), (1, 0, 1), (1, 1, 0)], [(0, 0, 1), (1, 0, 0)], [],
                                                    [], [(2, 0, 0), (5, 1, 0)], [(1, 0, 0), (3, 1, 0)]]
    assert [len(r["alleles"]) for r in doc["records"]] == [2, 2, 2, 2, 1, 3, 4]
    assert doc["records"][6]["alleles"][1] == dict(walk=[], text="G") and doc["records"][6]["alleles"][3] == dict(walk=[(7, 0), (8, 1)], text=None)
    d = H.parse_vcf(text)
    assert K.lib_arrays(d) == R.doc_arrays(doc)
    assert d.samples == ["A", "B"] and d.rec_line.tolist() == list(range(3, 10))
    # statuses of the odd ones: no AT, an allele beyond the walks, an empty walk
    names, paths = ["A#1#c", "B#1#c"], [[(1, 0), (2, 0)], [(7, 0), (8, 1)]]
    res = R.check(doc, names, paths, {1, 2, 7, 8})
    assert res["task_status"][-4:] == [R.NO_AT, R.NO_AT, R.NO_AT, R.FOUND_FWD]
    assert K.lib_texts(d, res, names)[0] == R.report_text(doc, res, names)


@pytest.mark.parametrize("text, message", [
    (vcf(["chr", "5", "x"]), "line 3: a record needs at least 8 columns, this one has 3"),
    (vcf(rec(), rec()[:-1]), "line 4: the #CHROM line names 2 sample columns, this record has 1"),
    (vcf(rec(pos="1e3")), "line 3: POS is no number: 1e3"),
    (vcf(rec(a="0|x")), "line 3: GT of sample column 0 is no genotype: 0|x"),
    (vcf(rec(a="0||1")), "line 3: GT of sample column 0 is no genotype: 0||1"),
    (vcf(rec(info="AT=>1>2,>1+3")), "line 3: AT walk 1 is no walk of [<>]id steps: >1+3"),
    (vcf(rec(info="AT=>1>,>3")), "line 3: AT walk 0 is no walk of [<>]id steps: >1>"),
    (vcf(rec(info="AT=>4294967295")), "line 3: AT walk 0 is no walk of [<>]id steps: >4294967295"),
    ("\t".join(rec()) + "\n" + HEAD, "line 1: a record in front of the #CHROM line"),
    (HEAD + HEAD, "line 4: a second #CHROM line"),
    ("#CHROM\tPOS\tID\n", "line 1: the #CHROM line needs at least 8 columns, this one has 3"),
])
def test_malformed_lines_are_refused_with_their_number(text, message):
    with pytest.raises(R.VcfError) as e:
        R.parse(text)
    assert str(e.value) == message
    for threads in (1, 3):
        with pytest.raises(RuntimeError) as e:
            H.parse_vcf(text, threads)
        assert str(e.value) == message


def test_the_first_of_several_malformed_lines_whatever_the_chunks():
    good = rec()
    records = [good] * 700 + [rec(pos="x")] + [good] * 500 + [rec(a="q")] + [good] * 300
    text = vcf(*records)
    for threads in (1, 2, 8):
        with pytest.raises(RuntimeError, match=r"^line 703: POS is no number: x$"):
            H.parse_vcf(text, threads)
    ok = vcf(*[rec(pos=str(k), ident=f"r{k}") for k in range(2000)]).replace("\n", "\r\n")
    d = H.parse_vcf(ok, 8)
    assert K.lib_arrays(d) == R.doc_arrays(R.parse(ok)) and d.n_records == 2000


def test_names_without_reference_prefixes_and_columns():
    import ctypes as C
    lib = H.load_lib()
    names = ["HG1#1#c", "HG1#2#c", "HG1#2#d", "plain", "HG2#3#c"]
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    err = C.create_string_buffer(512)
    nr = lib.povu_hip_vcf_names_make(len(names), arr, err, 512)
    assert nr
    n = nr.contents
    samples, slot_of_path, first, count, hap = R.slot_haps(names)
    assert n.refs.n_refs == 0 and [n.sample[k].decode() for k in range(n.refs.n_samples)] == samples == ["HG1", "plain", "HG2"]
    assert [n.slot_of_path[k] for k in range(len(names))] == slot_of_path == [0, 1, 1, 2, 3]
    assert [n.slot_hap[k] for k in range(n.refs.n_slots)] == [-1 if h is None else h for h in hap] == [1, 2, -1, 3]
    d = H.parse_vcf(HEAD.replace("\tA\tB", "\tHG2\tnobody\tHG1"))
    import numpy as np
    cf, cs = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
    assert lib.povu_hip_vcf_columns(d._p, nr, cf.ctypes.data, cs.ctypes.data) == 0
    assert cs.tolist() == [1, 0, 2] and cf[0] == 3 and cf[2] == 0
    lib.povu_hip_call_names_free(nr)


def test_report_text_first_failures():
    """A misspelled allele in front of the tasks of that allele, behind those of an earlier one; the hap number of a slot, 1 for a
    name without one and for a column nobody has."""
    names, paths = ["A#2#c", "B"], [[(1, 0), (2, 0), (4, 0)], [(1, 0), (3, 0), (4, 0)]]
    seqs = {1: "A", 2: "C", 3: "G", 4: "T"}
    head = HEAD.replace("\tA\tB", "\tA\tB\tZ")
    text = vcf(rec(info="AT=>2,>3", a="0", b="1") + ["."],           # valid, spelled whole
               rec(info="AT=>2,>3", ref="A", a="1", b="1") + ["."],  # REF misspelled, then A's allele 1 absent: misspelled first
               rec(info="AT=>2,>3", alt="A", a="0", b="0") + ["."],  # B's allele 0 absent, then ALT misspelled: the task first
               rec(info="AT=>1>2,>1>3", ref="AC", alt="AG", a="1", b="0") + ["1"],  # B's allele 0 absent first: no hap number, 1
               rec(info="AT=>1>2,>1>3", ref="AC", alt="AG", a="1", b="1") + ["."],  # A's allele 1 absent: hap number 2
               rec(info="AT=>1>2,>1>3", ref="AC", alt="AG", a="0", b="1") + ["1"],  # Z alone: no slot
               head=head)
    doc = R.parse(text)
    res = R.check(doc, names, paths, seqs.keys(), seqs, spelling=True)
    assert res["rec_invalid"] == [0, 1, 1, 1, 1, 1] and res["n_misspelled"] == 2
    assert res["allele_spell"][:6] == [R.SPELL_WHOLE, R.SPELL_WHOLE, R.SPELL_MISSPELLED, R.SPELL_WHOLE, R.SPELL_WHOLE, R.SPELL_MISSPELLED]
    assert res["allele_spell"][6:] == [R.SPELL_WHOLE] * 6
    want = ("rec_idx\tID\tPOS\tAT\tHap ID\tsample\treason\n"
            "1\tx\t5\t>2\t.\t.\tmisspelled\n"
            "2\tx\t5\t>2\t1\tB\tabsent\n"
            "3\tx\t5\t>1>2\t1\tB\tabsent\n"
            "4\tx\t5\t>1>3\t2\tA\tabsent\n"
            "5\tx\t5\t>1>3\t1\tZ\tno_slot\n")
    assert R.report_text(doc, res, names) == want
    d = H.parse_vcf(text)
    assert K.lib_texts(d, res, names) == (want, "Error rate: 83.33%\n")
    assert R.summary_text(doc, res) == "Error rate: 83.33%\n"


# ---- the rules as the device runs them, and the reader, under the sanitizers

@pytest.fixture(scope="module")
def vcfcheck_check():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povu_amd", "csrc"), "vcfcheck_check", "-s"])
    return os.path.join(ROOT, "build", "obj", "vcfcheck_check")


def run(exe, blocks):
    r = subprocess.run([exe], input="".join(blocks).encode(), capture_output=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()
    lines = r.stdout.decode().split("\n")
    assert lines[-2:] == ["vcfcheck_check: ok", ""]
    return lines[:-2]


def word(step):
    return step[0] << 1 | step[1]  # (segment ids as vertex indices)


def occ_block(w, paths, rev):
    off = [0]
    for p in paths:
        off.append(off[-1] + len(p))
    return "occ %d %d %d\n%s\n%s\n%s\n" % (rev, len(w), len(paths), " ".join(str(word(s)) for s in w), " ".join(map(str, off)),
                                           " ".join(str(word(s)) for p in paths for s in p))


def test_tokenizer_and_occurrence_rule_under_the_sanitizers(vcfcheck_check):
    rng = random.Random(11)
    blocks, want = [], []
    for text in [">1", "<22>3", ">1>2<3>44", "", ">", "1", ">1,", ">1>x", "<4294967294", ">4294967295", ">99999999999999999999999"]:
        blocks.append(f"walk {text}\n")
        w = R.walk_of(text)
        want.append("bad" if w is None else " ".join(f"{i}:{o}" for i, o in w))
    # the walk starts on the last step of a path and the next path begins with its other steps: absent; so for the reverse
    # reading; then random paths over few segments (many occurrences of every anchor, walks that reach the ends)
    cases = [([(1, 0), (2, 0), (3, 0)], [[(0, 0), (1, 0)], [(2, 0), (3, 0)]]),
             ([(3, 1), (2, 1), (1, 1)], [[(0, 0), (1, 0)], [(2, 0), (3, 0)]]),
             ([(1, 0)], [[(1, 0)], [], [(1, 1)]])]
    for _ in range(300):
        paths = [[(rng.randint(0, 3), rng.randint(0, 1)) for _ in range(rng.randint(0, 9))] for _ in range(rng.randint(1, 4))]
        src = rng.choice(paths)
        if src and rng.random() < 0.7:
            a = rng.randrange(len(src))
            w = src[a:a + rng.randint(1, 4)]
            if rng.random() < 0.5:
                w = R.flipped(w)
            if rng.random() < 0.3:
                w = w + [(rng.randint(0, 3), rng.randint(0, 1))]
        else:
            w = [(rng.randint(0, 3), rng.randint(0, 1)) for _ in range(rng.randint(1, 5))]
        cases.append((w, paths))
    n_hit = 0
    for w, paths in cases:
        for rev in (0, 1):
            blocks.append(occ_block(w, paths, rev))
            hits = [str(k) for k, p in enumerate(paths) if R.occurs(p, R.flipped(w) if rev else w)]
            n_hit += bool(hits)
            want.append(" ".join(hits))
    assert want[11:15] == ["", "", "", ""] and n_hit > 100
    assert run(vcfcheck_check, blocks) == want


def test_reader_under_the_sanitizers(vcfcheck_check):
    def dump(doc):
        a = R.doc_arrays(doc)
        out = [("S " + " ".join(a["sample"])).rstrip() if a["sample"] else "S"]
        for r in range(len(a["rec_line"])):
            out.append(f"R {a['rec_line'][r]} {a['rec_pos'][r]} {a['rec_id'][r]}")
            for k in range(a["allele_off"][r], a["allele_off"][r + 1]):
                steps = "".join(f" {a['step_id'][s]}:{a['step_or'][s]}" for s in range(a["step_off"][k], a["step_off"][k + 1]))
                out.append(f"A {a['allele_walk'][k]} {a['text'][a['text_off'][k]:a['text_off'][k + 1]]} |{steps}")
            for t in range(a["task_off"][r], a["task_off"][r + 1]):
                out.append(f"T {r} {a['task_allele'][t]} {a['task_col'][t]} {a['task_phase'][t]}")
        return out
    blocks, want = [], []
    texts = [K.fixture(f)[0] for f in K.FIXTURES]
    texts.append(vcf(*[rec(pos=str(k), a=f"{k % 3}|.", b="./1", info="AT=>1>2,<3,>9") for k in range(1500)]))
    texts += [vcf(rec(pos="-1")), vcf(rec(info="AT=>1<")), "", "#CHROM", vcf(rec()).rstrip("\n"), vcf(rec(a="", b=":"), rec(fmt="", a="", b=""))]
    for text in texts:
        for threads in (1, 5):
            raw = text.encode()
            blocks.append(f"vcf {threads} {len(raw)}\n{text}\n")
            try:
                want += dump(R.parse(text))
            except R.VcfError as e:
                want.append(f"error {e}")
    assert run(vcfcheck_check, blocks) == want

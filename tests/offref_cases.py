"""The graphs of the off-reference calls' tests (tests/golden/gfa/offref/, expected lines in tests/golden/offref_records.json)
read for the restatement: what test_offref_ref.py, test_offref_writer.py, test_offref_core.py and test_gpu_offref.py share."""
import json
import os

import oracle_lib as O
import vcf_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ISSUE = "inner-snp"  # the graph the feature was stated on
FIXTURE = os.path.join(GOLDEN, "gfa", "downstream_repetitive", "nested-child-inside-insertion.gfa")


def golden():
    return json.load(open(os.path.join(GOLDEN, "offref_records.json")))


def gfa_of(name):
    return os.path.join(GOLDEN, "gfa", "offref", name + ".gfa")


def pvst_texts(gfa, out):
    os.makedirs(out, exist_ok=True)
    n = O.decompose_gfa(gfa, str(out))
    return [open(os.path.join(out, f"{i}.pvst")).read() for i in range(1, n + 1) if os.path.exists(os.path.join(out, f"{i}.pvst"))]


def load(gfa, out):
    """(sites, names, paths, seqs, PVST texts) of a GFA, its PVSTs from the CPU oracle."""
    texts = pvst_texts(gfa, out)
    names, paths, seqs = V.read_gfa(gfa)
    return V.sites_of_pvst(texts), names, paths, seqs, texts


def records_of(text):
    return [ln for ln in text.splitlines() if not ln.startswith("#")]


def contigs_of(text):
    return [ln[len("##contig=<ID="):-1] for ln in text.splitlines() if ln.startswith("##contig")]

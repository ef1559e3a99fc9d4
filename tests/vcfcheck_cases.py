"""What the tests of the VCF checks share (test_vcfcheck_ref.py, test_gpu_vcfcheck.py, test_vcf_cli.py): the reference's nine
downstream_repetitive VCF fixtures (tests/golden/vcf/, their GFAs under tests/golden/gfa/, the expected statuses in
tests/golden/vcfcheck_expected.json), the library's document as the restatement's arrays, and the library's report text of a
restatement's result."""
import ctypes as C
import json
import os

import numpy as np

import vcfcheck_ref as R
from povu_amd import hip as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = [
    "subr-inversion-preservation/raw_graph.vcf",
    "subr-inversion-preservation/decomposed_passthrough.vcf",
    "vcfwave-complex-decomposition/raw_graph.vcf",
    "vcfwave-complex-decomposition/decomposed.vcf",
    "popped-parent-child-rescue/raw_graph.vcf",
    "popped-parent-child-rescue/top_level_only.vcf",
    "popped-parent-child-rescue/popped.vcf",
    "tandem-repeat-left-normalization/raw_graph.vcf",
    "tandem-repeat-left-normalization/left_normalized.vcf",
]


def expected():
    return json.load(open(os.path.join(GOLDEN, "vcfcheck_expected.json")))


def fixture(name):
    """(VCF text, path of its GFA)."""
    text = open(os.path.join(GOLDEN, "vcf", "downstream_repetitive", name)).read()
    return text, os.path.join(GOLDEN, "gfa", "downstream_repetitive", name.split("/")[0] + ".gfa")


def lib_arrays(d: "H.VcfDoc") -> dict:
    """A VcfDoc in the form of vcfcheck_ref.doc_arrays."""
    o = dict(sample=list(d.samples), rec_line=d.rec_line.tolist(), rec_pos=d.rec_pos.tolist(), rec_id=list(d.rec_id),
             text=bytes(d.text).decode())
    for k in ("allele_off", "task_off", "step_off", "text_off", "allele_walk", "step_id", "step_or", "task_record", "task_allele",
              "task_col", "task_phase"):
        o[k] = getattr(d, k).tolist()
    return o


def lib_texts(d: "H.VcfDoc", res: dict, names):
    """(report.tsv, summary.txt) as povu_hip_vcf_report_text writes them for the result `res` of vcfcheck_ref.check."""
    lib = H.load_lib()
    keep = {k: np.ascontiguousarray(res[k] + [0], dtype=dt) for k, dt in
            (("task_status", np.uint8), ("allele_spell", np.uint8), ("rec_invalid", np.uint8), ("rec_reason", np.uint8),
             ("rec_allele", np.uint32), ("rec_task", np.uint32))}
    rep = H._VcfReport()
    rep.n_records, rep.n_tasks, rep.n_alleles = d.n_records, d.n_tasks, d.n_alleles
    for k, a in keep.items():
        setattr(rep, k, a.ctypes.data_as(C.POINTER(C.c_uint8 if a.dtype == np.uint8 else C.c_uint32)))
    name_array = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    err = C.create_string_buffer(512)
    nr = lib.povu_hip_vcf_names_make(len(names), name_array, err, 512)
    assert nr, err.value
    try:
        return H._vcf_texts(lib, C.byref(rep), d._p, nr)
    finally:
        lib.povu_hip_call_names_free(nr)


def status_summary(doc: dict, res: dict) -> dict:
    """What vcfcheck_expected.json holds of a result: the tasks of every status and the tasks that were not found."""
    flat = [(r, a, c, j) for r, rec in enumerate(doc["records"]) for a, c, j in rec["tasks"]]
    return dict(n_records=len(doc["records"]), n_tasks=len(flat), n_status=res["n_status"],
                failing=[dict(record=r, allele=a, sample=doc["samples"][c], phase=j, status=R.STATUS_NAME[st])
                         for (r, a, c, j), st in zip(flat, res["task_status"]) if st > R.FOUND_REV])

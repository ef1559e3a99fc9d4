"""Device time of povu_hip_vcf_check (HipDecomposer.check_vcf) on the VCF of one of tools/time_calls.py's inputs: the plain call
of the workload is made and written as VCF (the device time of its third run is printed for comparison), the VCF is parsed once
(povu_hip_vcf_parse, --threads threads), and the check runs in each of the modes

    plain     every (allele, direction) searched, the tasks and records reduced
    spelling  the same with POVU_HIP_V_SPELLING: REF and ALT compared with the sequences of their walks
    tier2     plain with POVU_HIP_V_FORCE_TIER2: every search through the wave-per-unit kernel

One JSON line per mode and run: HIP-event time of the check (first upload to the last byte on the host), records, alleles,
tasks, the counters; then per mode a line with the median of the runs behind the warm-up runs and the tasks per second at it.

    python tools/time_vcfcheck.py --workload chain [--size 1.0] [--modes plain,spelling] [--warmup 2] [--runs 7] [--threads 16]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MODES = dict(plain={}, spelling=dict(spelling=True), tier2=dict(force_tier2=True))


def main():
    import time_calls as TC
    from povu_amd import HipDecomposer
    from povu_amd import hip as H
    from povu_amd import workloads as W
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(TC.DEFAULT_MODES), default="chain")
    ap.add_argument("--size", type=float, default=1.0, help="of the workload's own size")
    ap.add_argument("--modes", default="plain,spelling")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    modes = a.modes.split(",")
    for m in modes:
        if m not in MODES:
            ap.error("unknown mode " + m)
    g, p, seqs, ref = TC.workload(W, a.workload, a.size)
    d = HipDecomposer(0)
    d.upload(g)
    f = d.decompose(flags=H.F_NO_STAGE_TIMES)
    d.upload_paths(p)
    d.upload_sequences(seqs)
    for _ in range(3):  # (the third call's time: the arenas are warm)
        c = d.call(f, [ref])
    t0 = time.perf_counter()
    text = c.vcf_text(threads=a.threads)
    write_s = time.perf_counter() - t0
    call_ms, records = c.device_ms, c.n_records
    del c
    t0 = time.perf_counter()
    doc = H.parse_vcf(text, a.threads)
    parse_s = time.perf_counter() - t0
    print(json.dumps(dict(workload=a.workload, segments=g.n_vtx, paths=len(p), path_steps=p.n_steps, records=records,
                          call_device_ms=round(call_ms, 3), vcf_bytes=len(text), write_s=round(write_s, 2), parse_s=round(parse_s, 2),
                          alleles=doc.n_alleles, walk_steps=doc.n_steps, tasks=doc.n_tasks)), flush=True)
    del text
    for mode in modes:
        timed = []
        for run in range(a.warmup + a.runs):
            r = d.check_vcf(doc, **MODES[mode])
            row = dict(workload=a.workload, mode=mode, run=run, warmup=run < a.warmup, device_ms=round(r.device_ms, 3), tasks=r.n_tasks,
                       n_status=r.n_status, n_invalid=r.n_invalid, n_misspelled=r.n_misspelled, n_tier2=r.n_tier2)
            print(json.dumps(row), flush=True)
            if run >= a.warmup:
                timed.append(r.device_ms)
            del r
        med = statistics.median(timed)
        print(json.dumps(dict(workload=a.workload, mode=mode, median_device_ms=round(med, 3), min_device_ms=round(min(timed), 3),
                              max_device_ms=round(max(timed), 3), runs=len(timed), tasks_per_s=round(doc.n_tasks / (med * 1e-3)))), flush=True)
    d.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

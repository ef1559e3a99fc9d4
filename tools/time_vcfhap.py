"""Device time of povu_hip_vcf_haplotypes (HipDecomposer.compare_haplotypes) in REF-field mode on the inputs of
tools/time_vcfcmp.py: the wide cohort's VCF (131 sample columns) against its edited copy, as it stands and tiled to about
--records records on either side.  povu_hip_vcf_compare runs on the same documents in the same process as the yardstick.

One JSON line per input, call and run: HIP-event time (first upload to the last byte on the host), records, items, tasks,
windows, cells, the statuses; then per input and call a line with the median of the runs behind the warm-up runs.

    python tools/time_vcfhap.py [--records 1000000] [--warmup 2] [--runs 5] [--threads 16]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import cohort_cases as CC
    from povu_amd import HipDecomposer
    from povu_amd import hip as H
    from time_vcfcmp import edited, tiled
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1000000, help="of the tiled input (0: the cohort's VCF only)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    d = HipDecomposer(0)
    g, p = CC.wide_chain()
    d.upload(g)
    f = d.decompose()
    d.upload_paths(p)
    d.upload_sequences(CC.wide_sequences(g))
    text_a = d.call(f, [CC.REF_LOW]).vcf_text(date="00000000")
    text_b = edited(text_a)
    d.close()
    d = HipDecomposer(0)  # (a context that never sees a graph)
    n_records = H.parse_vcf(text_a).n_records
    for name, tiles in (("cohort", 1), ("tiled", -(-a.records // max(n_records, 1)))):
        if tiles < 1:
            continue
        t0 = time.perf_counter()
        docs = [H.parse_vcf(tiled(t, tiles) if tiles > 1 else t, a.threads) for t in (text_a, text_b)]
        prep_s = time.perf_counter() - t0
        for call in ("haplotypes", "compare"):
            timed = []
            for run in range(a.warmup + a.runs):
                t0 = time.perf_counter()
                c = d.compare_haplotypes(docs[0], docs[1]) if call == "haplotypes" else d.compare_vcfs(docs[0], docs[1])
                wall_s = time.perf_counter() - t0
                row = dict(input=name, call=call, run=run, warmup=run < a.warmup, device_ms=round(c.device_ms, 3), wall_s=round(wall_s, 3),
                           records=[docs[0].n_records, docs[1].n_records], tasks=[docs[0].n_tasks, docs[1].n_tasks],
                           items=[c.n_items_a, c.n_items_b], groups=c.n_groups, n_tier2=c.n_tier2)
                if call == "haplotypes":
                    row.update(windows=c.n_windows, cells=c.n_cells, inconsistent=c.n_inconsistent,
                               status=dict(zip(H.H_STATUS_NAMES, c.n_status)))
                else:
                    row.update(shared=c.n_shared, only_a=c.n_only_a, only_b=c.n_only_b)
                print(json.dumps(row), flush=True)
                if run >= a.warmup:
                    timed.append(c.device_ms)
                del c
            print(json.dumps(dict(input=name, call=call, prepare_s=round(prep_s, 2), median_device_ms=round(statistics.median(timed), 3),
                                  min_device_ms=round(min(timed), 3), max_device_ms=round(max(timed), 3), runs=len(timed))), flush=True)
        del docs
    d.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

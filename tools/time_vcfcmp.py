"""Device time of povu_hip_vcf_compare (HipDecomposer.compare_vcfs) on the wide cohort's VCF (tests/cohort_cases.py: 131 sample
columns) against an edited copy of it -- columns permuted, three renamed, two dropped, genotypes edited --, as it stands and
tiled: the records of both repeated, every copy further down its CHROM, until about --records records of 131 columns stand on
either side.

One JSON line per input and run: HIP-event time of the comparison (first upload to the last byte on the host), records, items,
tasks, groups, the counters; then per input a line with the median of the runs behind the warm-up runs.

    python tools/time_vcfcmp.py [--records 1000000] [--warmup 2] [--runs 5] [--threads 16]
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


def edited(text, seed=3):
    """The columns permuted, three renamed, two dropped, every fifth genotype of every third record moved to the next allele."""
    import numpy as np
    rng = np.random.default_rng(seed)
    lines = text.rstrip("\n").split("\n")
    at = next(k for k, ln in enumerate(lines) if ln.startswith("#CHROM"))
    head = lines[at].split("\t")
    order = [int(x) for x in rng.permutation(len(head) - 9)][:-2]
    names = [head[9 + c] for c in order]
    for k in (0, 64, 100):
        names[k] = "renamed" + str(k)
    out = lines[:at] + ["\t".join(head[:9] + names)]
    for r, ln in enumerate(lines[at + 1:]):
        f = ln.split("\t")
        n_alts = len(f[4].split(","))
        gts = [f[9 + c] for c in order]
        if r % 3 == 0:
            for k in range(0, len(gts), 5):
                gts[k] = "|".join("." if x == "." else str((int(x) + 1) % (n_alts + 1)) for x in gts[k].split("|"))
        out.append("\t".join(f[:9] + gts))
    return "\n".join(out) + "\n"


def tiled(text, tiles):
    """The records `tiles` times, copy t moved t * stride down its CHROM."""
    lines = text.rstrip("\n").split("\n")
    at = next(k for k, ln in enumerate(lines) if ln.startswith("#CHROM"))
    recs = [ln.split("\t", 2) for ln in lines[at + 1:]]
    stride = max(int(r[1]) for r in recs) + 1000
    out = lines[:at + 1]
    for t in range(tiles):
        out += [f"{c}\t{int(p) + t * stride}\t{rest}" for c, p, rest in recs]
    return "\n".join(out) + "\n"


def main():
    import cohort_cases as CC
    from povu_amd import HipDecomposer
    from povu_amd import hip as H
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
        timed = []
        for run in range(a.warmup + a.runs):
            t0 = time.perf_counter()
            c = d.compare_vcfs(docs[0], docs[1])
            wall_s = time.perf_counter() - t0
            row = dict(input=name, run=run, warmup=run < a.warmup, device_ms=round(c.device_ms, 3), wall_s=round(wall_s, 3),
                       records=[docs[0].n_records, docs[1].n_records], samples=[len(docs[0].samples), len(docs[1].samples)],
                       items=[c.n_items_a, c.n_items_b], tasks=[docs[0].n_tasks, docs[1].n_tasks], groups=c.n_groups, shared=c.n_shared,
                       only_a=c.n_only_a, only_b=c.n_only_b, common_samples=c.n_common_samples, tp=int(c.sample_tp.sum()),
                       fp=int(c.sample_fp.sum()), fn=int(c.sample_fn.sum()), gteq=int(c.sample_gteq.sum()), n_tier2=c.n_tier2)
            print(json.dumps(row), flush=True)
            if run >= a.warmup:
                timed.append(c.device_ms)
            del c
        print(json.dumps(dict(input=name, prepare_s=round(prep_s, 2), median_device_ms=round(statistics.median(timed), 3),
                              min_device_ms=round(min(timed), 3), max_device_ms=round(max(timed), 3), runs=len(timed))), flush=True)
        del docs
    d.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Device time of the left-normalised call (HipDecomposer.call under the `left-normalized` profile, INTEGRATION.md
"Left-normalised calls") against the raw call of the same build on the same input: a tandem_indels graph
(workloads.tandem_indels / tandem_haplotypes: an indel of one period at the right end of every tandem repeat) with PanSN
haplotypes and one reference.  One JSON line per mode and run: HIP-event time of the call (query upload to the last byte on
the host), records, spelled bytes, the normalisation's counters; then per mode a summary line with the median of the runs
behind the warm-up runs, and for `normalized` its difference to the raw call's median.  On a build without the profile
(the parent commit) `--only raw` gives the raw call's time alone.

Every mode runs in a child process of its own under its own time limit, one after the other; after a child that fails or
runs out of time nothing more is started.

    python tools/time_norm.py [--units 100000] [--haps 8] [--warmup 2] [--runs 7] [--limit 300] [--only raw|normalized]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ("raw", "normalized")


def child(a):
    from povu_amd import HipDecomposer
    from povu_amd import hip as H
    from povu_amd import workloads as W

    t0 = time.perf_counter()
    g, seqs = W.tandem_indels(a.units, 1)
    p = W.tandem_haplotypes(a.units, 1, a.haps)
    gen_s = time.perf_counter() - t0
    d = HipDecomposer(0)
    d.upload(g)
    f = d.decompose(flags=H.F_NO_STAGE_TIMES)
    d.upload_paths(p)
    d.upload_sequences(seqs)
    kw = dict(raw={}, normalized=dict(profile="left-normalized"))[a.child]
    for run in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        c = d.call(f, ["hap0#"], **kw)
        wall = (time.perf_counter() - t0) * 1e3
        print(json.dumps(dict(
            mode=a.child, run=run, warmup=run < a.warmup, segments=g.n_vtx, links=g.n_links, units=a.units, paths=len(p),
            path_steps=p.n_steps, records=c.n_records, spelled_bytes=c.n_seq_bytes, device_ms=round(c.device_ms, 3),
            wall_ms=round(wall, 2), generate_s=round(gen_s, 1), normalized=getattr(c, "n_normalized", 0),
            max_shift=getattr(c, "max_shift", 0), norm_compared=getattr(c, "n_norm_compared", 0))), flush=True)
        del c
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=100000)
    ap.add_argument("--haps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--limit", type=int, default=300, help="seconds a mode may take")
    ap.add_argument("--only", choices=MODES)
    ap.add_argument("--child", choices=MODES, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    median = {}
    for mode in MODES if a.only is None else (a.only,):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--units", str(a.units),
               "--haps", str(a.haps), "--warmup", str(a.warmup), "--runs", str(a.runs)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(json.dumps(dict(mode=mode, failed=r.returncode)), flush=True)
            return 1  # (nothing more is started on the GPU)
        rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        timed = [x["device_ms"] for x in rows if not x["warmup"]]
        median[mode] = statistics.median(timed)
        out = dict(mode=mode, median_device_ms=round(median[mode], 3), min_device_ms=min(timed), max_device_ms=max(timed), runs=len(timed),
                   records=rows[-1]["records"], norm_compared=rows[-1]["norm_compared"])
        if mode == "normalized" and "raw" in median:
            out.update(extra_ms_over_raw=round(median[mode] - median["raw"], 3), ratio_to_raw=round(median[mode] / median["raw"], 3))
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

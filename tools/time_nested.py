"""Device time of the nested calls (HipDecomposer.call with T_NESTED and under the `popped` profile) against the plain call
on the same input: a skip_nested graph (workloads.skip_nested / skip_haplotypes: units with a skip link around a chain of
sub-units, INTEGRATION.md "Nested calls") with PanSN haplotypes, one reference and random sequences.  One JSON line per
mode and run: HIP-event time of the call (query upload to the last byte on the host), records, spelled bytes, the nested
counters; after the runs of a mode other than `plain`, its ratio to the plain call's best run.

Every mode runs in a child process of its own under its own time limit, one after the other; after a child that fails or
runs out of time nothing more is started.

    python tools/time_nested.py [--segments 1e6] [--depth 2] [--haps 64] [--runs 3] [--max-length 64] [--limit 300]
"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ("plain", "nested", "popped")


def child(a):
    from povu_amd import HipDecomposer
    from povu_amd import hip as H
    from povu_amd import workloads as W

    size = len(W._skip_template(a.depth, 2)[0])
    units = max(2, int(a.segments / size) + 1)
    t0 = time.perf_counter()
    g = W.skip_nested(units, a.depth)
    p = W.skip_haplotypes(units, a.depth, a.haps, seed=1)
    seqs = W.random_sequences(g, 5, max_len=16)
    gen_s = time.perf_counter() - t0
    d = HipDecomposer(0)
    d.upload(g)
    f = d.decompose(flags=H.F_NO_STAGE_TIMES)
    d.upload_paths(p)
    d.upload_sequences(seqs)
    kw = dict(plain={}, nested=dict(flags=H.T_NESTED),
              popped=dict(profile="popped", max_level=0, max_ref_length=a.max_length, max_allele_length=a.max_length))[a.child]
    for run in range(a.runs):
        t0 = time.perf_counter()
        c = d.call(f, ["hap0#"], **kw)
        wall = (time.perf_counter() - t0) * 1e3
        print(json.dumps(dict(
            mode=a.child, run=run, segments=g.n_vtx, links=g.n_links, units=units, depth=a.depth, paths=len(p),
            path_steps=p.n_steps, records=c.n_records, slots=c.n_slots, spelled_bytes=c.n_seq_bytes, at_bytes=c.n_at_bytes,
            device_ms=round(c.device_ms, 2), wall_ms=round(wall, 2), generate_s=round(gen_s, 1), enclosed=c.n_enclosed,
            collapsed_sites=c.n_collapsed_sites, popped=c.n_popped, rescued=c.n_rescued,
            max_alleles=int(c.n_alleles.max()) if c.n_records else 0)), flush=True)
        del c
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=float, default=1e6)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--haps", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--max-length", type=int, default=64, help="popped: max_ref_length and max_allele_length")
    ap.add_argument("--limit", type=int, default=300, help="seconds a mode may take")
    ap.add_argument("--only", choices=MODES)
    ap.add_argument("--child", choices=MODES, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    best = {}
    for mode in MODES if a.only is None else (a.only,):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--segments",
               str(a.segments), "--depth", str(a.depth), "--haps", str(a.haps), "--runs", str(a.runs), "--max-length", str(a.max_length)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(json.dumps(dict(mode=mode, failed=r.returncode)), flush=True)
            return 1  # (nothing more is started on the GPU)
        rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        best[mode] = min(rows, key=lambda x: x["device_ms"])
        if mode != "plain" and "plain" in best:
            print(json.dumps(dict(mode=mode, device_ms_over_plain=round(best[mode]["device_ms"] / best["plain"]["device_ms"], 3),
                                  spelled_bytes_over_plain=round(best[mode]["spelled_bytes"] / max(1, best["plain"]["spelled_bytes"]), 4))),
                  flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

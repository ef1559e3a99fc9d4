"""Device time of povu_hip_call (HipDecomposer.call) on two graphs with 32 haplotypes and one reference: the chain of bubbles
with closed-form haplotypes (workloads.chain_haplotypes, a quarter of them written reversed) and an HPRC-shaped graph with
random-walk paths, random sequences on both (workloads.random_sequences).  One JSON line per graph and run: HIP-event time of
the call (query upload to the last byte on the host), records per second, spelled bytes, and the bytes of a traffic model
against the 8 TB/s HBM peak.

The model (kept here, stated in DESIGN.md): the traversal pipeline's count and emit passes (tools/time_traversals.py: 24 B per path step; its scans are
not counted, a lower bound); per reference step 4 B read and 8 B length gathered, written, scanned and read back (40 B), and its
boundary-table offsets (8 B); per record its GT row (2 B a slot) and its slot-table reads (8 B a slot); every spelled base
read and written (2 B) and every AT byte written.

    python tools/time_call.py [--scale 1.0] [--haps 32] [--runs 3] [--only chain|hprc]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from povu_amd import HipDecomposer  # noqa: E402
from povu_amd import hip as H  # noqa: E402
from povu_amd import workloads as W  # noqa: E402

HBM_PEAK = 8e12


def graphs(scale, haps, only):
    if only in (None, "chain"):
        k = max(100, int(1e6 * scale))
        yield "chain", lambda: W.chain_of_bubbles(k), lambda g: W.chain_haplotypes(k, haps, seed=1)
    if only in (None, "hprc"):
        yield "hprc", (lambda: W.hprc_shaped([max(1000, int(6e5 * scale)), max(1000, int(3e5 * scale))], seed=3, tiny=5)), \
            lambda g: W.random_walk_paths(g, haps, max(1000, int(6e5 * scale)), seed=4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--haps", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=["chain", "hprc"])
    a = ap.parse_args()
    d = HipDecomposer(0)
    for name, make, make_paths in graphs(a.scale, a.haps, a.only):
        t0 = time.perf_counter()
        g = make()
        p = W.pansn(make_paths(g), samples=a.haps)  # one haploid slot per path; sample0 is the reference
        seqs = W.random_sequences(g, 5, max_len=300)
        gen_s = time.perf_counter() - t0
        d.upload(g)
        f = d.decompose(flags=H.F_NO_STAGE_TIMES)
        d.upload_paths(p)
        d.upload_sequences(seqs)
        ref_steps = int(p.off[1] - p.off[0])
        for run in range(a.runs):
            t0 = time.perf_counter()
            c = d.call(f, ["sample0#"])
            wall = (time.perf_counter() - t0) * 1e3
            n = c.n_records
            b = (p.n_steps * 24 + ref_steps * 48 + n * c.n_slots * 10 + 2 * c.n_seq_bytes + c.n_at_bytes)
            ms = c.device_ms
            print(json.dumps(dict(
                graph=name, run=run, segments=g.n_vtx, links=g.n_links, paths=len(p), path_steps=p.n_steps,
                reference_steps=ref_steps, records=n, slots=c.n_slots, spelled_bytes=c.n_seq_bytes, at_bytes=c.n_at_bytes,
                device_ms=round(ms, 2), wall_ms=round(wall, 2), generate_s=round(gen_s, 1),
                records_per_s=round(n / (ms * 1e-3), 0) if ms > 0 else None, model_bytes=b,
                model_tb_per_s=round(b / (ms * 1e-3) / 1e12, 3) if ms > 0 else None,
                model_of_peak=round(b / (ms * 1e-3) / HBM_PEAK, 4) if ms > 0 else None)), flush=True)
            del c
        del f, p, g


if __name__ == "__main__":
    main()

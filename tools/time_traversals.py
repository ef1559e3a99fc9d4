"""Device time of povu_hip_forest_traversals (HipDecomposer.traversals) on three graphs with paths: the chain of bubbles with
closed-form haplotypes (workloads.chain_haplotypes, a quarter of them written reversed), nested towers with random-walk paths,
and an HPRC-shaped graph with random-walk paths.  One JSON line per graph and run: HIP-event time of the call (query upload
to the last byte on the host), path steps per second, and the bytes of a traffic model against the 8 TB/s HBM peak.

The model (kept here, stated in DESIGN.md): the count and emit passes each stream every path step (4 B) and gather its two
boundary-table offsets (8 B); every scan reads the steps it looks at (4 B), and a closed scan reads them again to hash them.
Scanned steps are taken as the traversals' own steps (the steps of scans that do not close are not counted: a lower bound).

    python tools/time_traversals.py [--scale 1.0] [--haps 32] [--runs 3] [--only chain|towers|hprc]
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
        k = max(100, int(1e8 * scale / 3))
        yield "chain", lambda: W.chain_of_bubbles(k), lambda g: W.chain_haplotypes(k, haps, seed=1)
    if only in (None, "towers"):
        t = max(10, int(2e6 * scale))
        yield "towers", lambda: W.nested_towers(12, t), lambda g: W.random_walk_paths(g, haps, max(1000, int(2e6 * scale)), seed=2)
    if only in (None, "hprc"):
        yield "hprc", (lambda: W.hprc_shaped([max(1000, int(2e6 * scale)), max(1000, int(1e6 * scale))], seed=3, tiny=5)), \
            lambda g: W.random_walk_paths(g, haps, max(1000, int(2e6 * scale)), seed=4)


def model_bytes(n_steps, scanned):
    return n_steps * (4 + 8) * 2 + scanned * 4 * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--haps", type=int, default=32)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=["chain", "towers", "hprc"])
    a = ap.parse_args()
    d = HipDecomposer(0)
    for name, make, make_paths in graphs(a.scale, a.haps, a.only):
        t0 = time.perf_counter()
        g = make()
        p = make_paths(g)
        gen_s = time.perf_counter() - t0
        d.upload(g)
        f = d.decompose(flags=H.F_NO_STAGE_TIMES)
        t0 = time.perf_counter()
        d.upload_paths(p)
        up_ms = (time.perf_counter() - t0) * 1e3
        for run in range(a.runs):
            t0 = time.perf_counter()
            t = d.traversals(f)
            wall = (time.perf_counter() - t0) * 1e3
            scanned = int((t.last.astype(np.int64) - t.first.astype(np.int64) + 1).sum())
            b = model_bytes(p.n_steps, scanned)
            st = t.status
            print(json.dumps(dict(
                graph=name, run=run, segments=g.n_vtx, links=g.n_links, paths=len(p), path_steps=p.n_steps, queries=t.n_queries,
                traversals=t.n_traversals, alleles=t.n_alleles, allele_steps=t.n_steps, tier2_scans=t.n_tier2,
                hash_splits=t.n_hash_splits, device_ms=round(t.device_ms, 2), wall_ms=round(wall, 2),
                paths_upload_wall_ms=round(up_ms, 1), generate_s=round(gen_s, 1),
                path_steps_per_s=round(p.n_steps / (t.device_ms * 1e-3), 0) if t.device_ms > 0 else None,
                model_bytes=b, model_tb_per_s=round(b / (t.device_ms * 1e-3) / 1e12, 3) if t.device_ms > 0 else None,
                model_of_peak=round(b / (t.device_ms * 1e-3) / HBM_PEAK, 4) if t.device_ms > 0 else None,
                long=int(np.count_nonzero(st & H.TRAV_LONG)), stray=int(np.count_nonzero(st & H.TRAV_STRAY)),
                open=int(np.count_nonzero(st & H.TRAV_OPEN)))), flush=True)
            del t
        del f, p, g
    d.close()


if __name__ == "__main__":
    main()

"""Device time of povu_hip_forest_walks (HipDecomposer.walks) on the bench headline graph (workloads.hprc_whole_genome) and
on the tangled graph of bench.py, with the default caps: HIP-event time of the call (query upload to the last byte on the
host), queries per tier and how many queries hit each cap.  One JSON line per graph and run.

    python tools/time_walks.py [--scale 1.0] [--runs 3] [--only hprc-wg|tangled]
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


def graphs(scale, only):
    if only in (None, "hprc-wg"):
        yield "hprc-wg", lambda: W.hprc_whole_genome(1e8 * scale)
    if only in (None, "tangled"):
        yield "tangled", lambda: W.hprc_tangled(max(1000, int(3e6 * scale)), tangle_every=100000, max_tangle=300000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=["hprc-wg", "tangled"])
    a = ap.parse_args()
    d = HipDecomposer(0)
    for name, make in graphs(a.scale, a.only):
        g = make()
        d.upload(g)
        f = d.decompose(flags=H.F_NO_STAGE_TIMES)
        for run in range(a.runs):
            t0 = time.perf_counter()
            w = d.walks(f)
            wall = (time.perf_counter() - t0) * 1e3
            st = w.status
            nw = np.diff(w.walk_off.astype(np.int64))
            print(json.dumps(dict(
                graph=name, run=run, segments=g.n_vtx, links=g.n_links, queries=w.n_queries, walks=w.n_walks, steps=w.n_steps,
                device_ms=round(w.device_ms, 2), wall_ms=round(wall, 2), tier1_queries=w.n_queries - w.n_tier2,
                tier2_queries=w.n_tier2, more=int(np.count_nonzero(st & H.WALK_MORE)),
                long=int(np.count_nonzero(st & H.WALK_LONG)), budget=int(np.count_nonzero(st & H.WALK_BUDGET)),
                no_walk=int(np.count_nonzero(nw == 0)), max_walk_steps=int(np.diff(w.step_off.astype(np.int64)).max(initial=0)))),
                flush=True)
            del w
        del f
    d.close()


if __name__ == "__main__":
    main()

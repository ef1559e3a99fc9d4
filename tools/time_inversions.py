"""Device time of povu_hip_call (HipDecomposer.call) with and without POVU_HIP_T_INVERSIONS on the same resident input: the
chain of bubbles with closed-form haplotypes (the traversal timing workload, tools/time_traversals.py) once with no step in
the opposite orientation at all (every haplotype written forward) and once with workloads.inverted_haplotypes applied (every
haplotype but the reference gets intervals walked backwards; with --copies some haplotypes are copies of the reference, so
that whole intervals are runs).  One JSON line per input, flag and run: HIP-event time of the call, records, the inversion
counters.

    python tools/time_inversions.py [--scale 0.01] [--haps 32] [--runs 5] [--intervals 1000] [--max-len 2000] [--copies 4]
                                    [--package-root <another checkout>]
"""
import argparse
import json
import os
import sys
import time

import importlib.util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(package_root):
    """(HipDecomposer, hip module, this tree's workloads): the library of another checkout with --package-root (the yardstick
    of the call without the flag at another commit), the inputs always this tree's."""
    spec = importlib.util.spec_from_file_location("time_inversions_workloads", os.path.join(ROOT, "povu_amd", "workloads.py"))
    w = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = w
    spec.loader.exec_module(w)
    sys.path.insert(0, os.path.abspath(package_root) if package_root else ROOT)
    from povu_amd import HipDecomposer
    from povu_amd import hip
    return HipDecomposer, hip, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.01)
    ap.add_argument("--haps", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--intervals", type=int, default=1000)
    ap.add_argument("--max-len", type=int, default=2000)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--package-root", help="import povu_amd from this checkout; a build without the flag is timed without it only")
    a = ap.parse_args()
    HipDecomposer, H, W = _load(a.package_root)
    with_flag = getattr(H, "T_INVERSIONS", None)
    k = max(100, int(1e8 * a.scale / 3))
    g = W.chain_of_bubbles(k)
    base = W.chain_haplotypes(k, a.haps, seed=1, reverse_every=0)
    cut = lambda j: (base.ids[int(base.off[j]):int(base.off[j + 1])], base.rev[int(base.off[j]):int(base.off[j + 1])])  # noqa: E731
    copied = W._paths(base.names, [cut(0 if 1 <= j <= a.copies else j) for j in range(a.haps)])
    inputs = [("forward_only", W.pansn(base, samples=a.haps)),
              ("inverted", W.pansn(W.inverted_haplotypes(copied, a.intervals, 2, a.max_len, 2, keep=(0,)), samples=a.haps))]
    d = HipDecomposer(0)
    d.upload(g)
    f = d.decompose(flags=H.F_NO_STAGE_TIMES)
    d.upload_sequences(W.random_sequences(g, 1, max_len=30))
    for name, p in inputs:
        d.upload_paths(p)
        for flags in (0,) if with_flag is None else (0, with_flag):
            for run in range(a.runs):
                t0 = time.perf_counter()
                c = d.call(f, ["sample0#"], flags=flags)
                wall = (time.perf_counter() - t0) * 1e3
                print(json.dumps(dict(input=name, inversions=bool(flags), run=run, segments=g.n_vtx, paths=len(p),
                                      path_steps=p.n_steps, records=c.n_records, inv_records=getattr(c, "n_inv_records", 0),
                                      inv_heads=getattr(c, "n_inv_heads", 0), inv_long=getattr(c, "n_inv_long", 0),
                                      inv_tier2=getattr(c, "n_inv_tier2", 0),
                                      longest_run=int(c.n_steps.max()) if flags and c.n_records else 0,
                                      device_ms=round(c.device_ms, 3), wall_ms=round(wall, 2))), flush=True)
                del c
    d.close()


if __name__ == "__main__":
    main()

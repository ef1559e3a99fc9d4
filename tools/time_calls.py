"""Device time of povu_hip_call (HipDecomposer.call) in its modes on one of eight inputs, each at the size it has always been
timed at:

    chain     the chain of bubbles with 32 closed-form haplotypes, a quarter written reversed (workloads.chain_haplotypes),
              random sequences of up to 300 bases; 1e6 bubbles
    inverted  the chain with every haplotype written forward, four of them copies of the reference, and
              workloads.inverted_haplotypes applied (1000 intervals of up to 2000 steps walked backwards); 333333 bubbles
    skip      workloads.skip_nested / skip_haplotypes at depth 2 with 64 haplotypes (INTEGRATION.md "Nested calls"); 1e6 segments
    tandem    workloads.tandem_indels / tandem_haplotypes with 8 haplotypes (an indel of one period at the right end of every
              tandem repeat, INTEGRATION.md "Left-normalised calls"); 100000 units
    complex   workloads.complex_alleles / complex_haplotypes with 8 haplotypes (bubbles of several small edits, INTEGRATION.md
              "Decomposed calls"); 100000 units
    insertions workloads.insertion_units / insertion_haplotypes with 64 haplotypes (a SNP inside an insertion the reference does
              not have, INTEGRATION.md "Off-reference calls"); 125000 units, 1e6 segments
    looped    workloads.vntr_haplotypes with 32 haplotypes of 1 .. 6 laps a site, every fourth walking backwards (loop sites,
              INTEGRATION.md "Untangled calls"); 100000 sites, 5e5 segments
    braid     workloads.braid / braid_haplotypes with 64 near-equal haplotypes (sites of 24 layers of 2 parallel segments that the
              PVST does not split, a layer redrawn with probability 0.02: one changed layer is 23 / 25 similar, two are 22 / 26;
              INTEGRATION.md "Clustered calls"); 20000 sites, 1e6 segments

and in any of the modes plain, inversions (T_INVERSIONS), nested (T_NESTED), popped (profile `popped`, max_level 0, both length
limits --max-length), normalized (profile `left-normalized`), decomposed (profile `decomposed`), merged (the same with T_MERGE:
equal primitives merged; its time less that of decomposed is the merging step's) and decomposed-tier2 (decomposed with
T_FORCE_TIER2: every aligned pair through the striped kernel, for the cells per second of that tier; asked for by name
only), offref (T_OFFREF: the sites no reference path crosses too; its time less that of plain is the step's) and untangled
(T_UNTANGLE: the laps of every haplotype aligned with the reference's; its time less that of plain is the step's) and region
(asked for by name only: the plain call restricted to the middle 1 % of the first reference path's bases, INTEGRATION.md "Region
calls"; the sites outside lose their scans) and cluster (the clustered call at T = 900000, INTEGRATION.md "Clustered calls"; its
time less that of plain is the step's; `alts` counts the ALTs written) and spanning / popped-spanning (asked for by name only:
nested and popped with T_SPANNING, INTEGRATION.md "Spanning alleles"; their time less that of nested / popped is the option's);
without --modes those the input was made for.  One JSON line
per mode and run: HIP-event time of the call (query upload to the last byte on the host), records, spelled bytes, the
counters of the mode, and the host time of the VCF writer over these calls on one thread (vcf_ms, with the bytes and the MD5 of
its text); then per mode a line with the median of the runs behind the warm-up runs.

Every mode runs in a child process of its own under its own time limit, one after the other; after a child that fails or
runs out of time nothing more is started.  --package-root times the library of another checkout on this tree's inputs (only
keyword arguments of HipDecomposer.call that every build with the mode has are used).

    python tools/time_calls.py --workload chain|inverted|skip|tandem|complex|insertions|looped|braid [--modes plain,nested] [--size 1.0] [--warmup 2] [--runs 7]
                               [--max-length 64] [--limit 300] [--package-root <another checkout>]
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = ("plain", "inversions", "nested", "popped", "normalized", "decomposed", "merged", "decomposed-tier2", "offref", "untangled", "region", "cluster",
         "spanning", "popped-spanning")
DEFAULT_MODES = dict(chain=("plain",), inverted=("plain", "inversions"), skip=("plain", "nested", "popped"), tandem=("plain", "normalized"),
                     complex=("plain", "decomposed", "merged"), insertions=("plain", "offref"), looped=("plain", "untangled"), braid=("plain", "cluster"))


def _load(package_root):
    """(HipDecomposer, hip module, this tree's workloads): the library of another checkout with --package-root, the inputs
    always this tree's."""
    spec = importlib.util.spec_from_file_location("time_calls_workloads", os.path.join(ROOT, "povu_amd", "workloads.py"))
    w = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = w
    spec.loader.exec_module(w)
    sys.path.insert(0, os.path.abspath(package_root) if package_root else ROOT)
    from povu_amd import HipDecomposer
    from povu_amd import hip
    return HipDecomposer, hip, w


def workload(W, name, size):
    """(graph, paths, sequences, reference prefix)"""
    if name == "chain":
        k = max(100, int(1e6 * size))
        g = W.chain_of_bubbles(k)
        return g, W.pansn(W.chain_haplotypes(k, 32, seed=1), samples=32), W.random_sequences(g, 5, max_len=300), "sample0#"
    if name == "inverted":
        k = max(100, int(1e8 * 0.01 * size / 3))
        g = W.chain_of_bubbles(k)
        base = W.chain_haplotypes(k, 32, seed=1, reverse_every=0)
        cut = lambda j: (base.ids[int(base.off[j]):int(base.off[j + 1])], base.rev[int(base.off[j]):int(base.off[j + 1])])  # noqa: E731
        copied = W._paths(base.names, [cut(0 if 1 <= j <= 4 else j) for j in range(32)])
        p = W.pansn(W.inverted_haplotypes(copied, 1000, 2, 2000, 2, keep=(0,)), samples=32)
        return g, p, W.random_sequences(g, 1, max_len=30), "sample0#"
    if name == "skip":
        units = max(2, int(1e6 * size / len(W._skip_template(2, 2)[0])) + 1)
        g = W.skip_nested(units, 2)
        return g, W.skip_haplotypes(units, 2, 64, seed=1), W.random_sequences(g, 5, max_len=16), "hap0#"
    if name == "insertions":
        units = max(2, int(125000 * size))
        g = W.insertion_units(units)
        return g, W.insertion_haplotypes(units, 64, seed=1), W.random_sequences(g, 5, max_len=16), "hap0#"
    if name == "looped":
        sites = max(2, int(100000 * size))
        g, p = W.vntr_haplotypes(sites, 32, 6, 1, reverse_every=4)
        return g, p, W.random_sequences(g, 5, max_len=16), "hap0#"
    if name == "braid":
        sites = max(2, int(20000 * size))
        g = W.braid(sites, 24, 2, seed=1)
        return g, W.braid_haplotypes(sites, 24, 2, 64, seed=1, mutate=0.02), W.random_sequences(g, 5, max_len=16), "hap0#"
    if name == "complex":
        units = max(2, int(100000 * size))
        g, seqs = W.complex_alleles(units, 1)
        return g, W.complex_haplotypes(units, 1, 8), seqs, "hap0#"
    units = max(2, int(100000 * size))
    g, seqs = W.tandem_indels(units, 1)
    return g, W.tandem_haplotypes(units, 1, 8), seqs, "hap0#"


def middle_region(g, p, seqs, ref):
    """(name, start, end): the middle 1 % of the bases of the first path whose name starts with `ref`."""
    import numpy as np
    k = next(i for i, n in enumerate(p.names) if n.startswith(ref))
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    ids = np.asarray(p.ids[int(p.off[k]):int(p.off[k + 1])])
    total = int(lens[np.searchsorted(np.asarray(g.vid), ids)].sum())
    start = 1 + (total * 99) // 200
    return p.names[k], start, max(start + 1, start + total // 100)


def writer(c, H):
    """(milliseconds, bytes, MD5) of povu_hip_calls_vcf_profile over the calls `c`, the copy into Python left out"""
    import ctypes as C
    import hashlib
    ln = C.c_size_t(0)
    t0 = time.perf_counter()
    p = c._lib.povu_hip_calls_vcf_profile(c._p, c._sites._p, c._names_rec, c._name_array, b"00000000", None, 1, H.PROFILES[c.profile], C.byref(ln))
    ms = (time.perf_counter() - t0) * 1e3
    digest = hashlib.md5(C.string_at(p, ln.value)).hexdigest()
    c._lib.povu_hip_buffer_free(p)
    return ms, ln.value, digest


def child(a):
    HipDecomposer, H, W = _load(a.package_root)
    t0 = time.perf_counter()
    g, p, seqs, ref = workload(W, a.workload, a.size)
    gen_s = time.perf_counter() - t0
    d = HipDecomposer(0)
    d.upload(g)
    f = d.decompose(flags=H.F_NO_STAGE_TIMES)
    d.upload_paths(p)
    d.upload_sequences(seqs)
    kw = dict(plain=lambda: {}, inversions=lambda: dict(flags=H.T_INVERSIONS), nested=lambda: dict(flags=H.T_NESTED),
              popped=lambda: dict(profile="popped", max_level=0, max_ref_length=a.max_length, max_allele_length=a.max_length),
              normalized=lambda: dict(profile="left-normalized"), decomposed=lambda: dict(profile="decomposed"),
              merged=lambda: dict(profile="decomposed", flags=H.T_MERGE), offref=lambda: dict(flags=H.T_OFFREF), untangled=lambda: dict(flags=H.T_UNTANGLE),
              region=lambda: dict(regions=[middle_region(g, p, seqs, ref)]), cluster=lambda: dict(cluster=900000),
              spanning=lambda: dict(flags=H.T_NESTED | H.T_SPANNING),
              **{"decomposed-tier2": lambda: dict(profile="decomposed", flags=H.T_FORCE_TIER2),
                 "popped-spanning": lambda: dict(profile="popped", flags=H.T_SPANNING, max_level=0, max_ref_length=a.max_length,
                                                 max_allele_length=a.max_length)})[a.child]()
    counters = ("n_inv_records", "n_inv_tier2", "n_enclosed", "n_collapsed_sites", "n_popped", "n_rescued", "n_normalized", "max_shift",
                "n_norm_compared", "n_rows", "n_decomposed_alts", "n_passthrough_alts", "n_prim_tier2", "n_prim_cells", "n_mrows",
                "n_merged_groups", "n_merged_members", "n_merge_splits", "n_ref_consistent", "n_gt_conflicts", "n_offref_sites", "n_offref_records", "n_offref_hosted",
                "n_unt_tasks", "n_unt_records", "n_unt_missing", "n_unt_extra", "n_unt_fallback", "n_regions", "n_region_sites", "n_region_masked",
                "n_region_dropped") + tuple(getattr(H, "CLUSTER_COUNTERS", ())) + tuple(getattr(H, "SPAN_COUNTERS", ()))
    for run in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        c = d.call(f, [ref], **kw)
        wall = (time.perf_counter() - t0) * 1e3
        vcf_ms, vcf_bytes, vcf_md5 = writer(c, H)
        print(json.dumps(dict(
            workload=a.workload, mode=a.child, run=run, warmup=run < a.warmup, segments=g.n_vtx, links=g.n_links, paths=len(p),
            path_steps=p.n_steps, records=c.n_records, slots=c.n_slots, spelled_bytes=c.n_seq_bytes, at_bytes=c.n_at_bytes,
            alts=int(c.ac_off[-1]) if c.n_records else 0, device_ms=round(c.device_ms, 3), wall_ms=round(wall, 2), generate_s=round(gen_s, 1),
            vcf_ms=round(vcf_ms, 2), vcf_bytes=vcf_bytes, vcf_md5=vcf_md5,
            **{k: int(getattr(c, k, 0)) for k in counters})), flush=True)
        del c
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(DEFAULT_MODES), required=True)
    ap.add_argument("--modes", help="comma-separated, of " + ",".join(MODES))
    ap.add_argument("--size", type=float, default=1.0, help="of the workload's own size")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--max-length", type=int, default=64, help="popped: max_ref_length and max_allele_length")
    ap.add_argument("--limit", type=int, default=300, help="seconds a mode may take")
    ap.add_argument("--package-root", help="import povu_amd from this checkout")
    ap.add_argument("--child", choices=MODES, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    modes = tuple(a.modes.split(",")) if a.modes else DEFAULT_MODES[a.workload]
    for mode in modes:
        if mode not in MODES:
            ap.error("unknown mode " + mode)
    for mode in modes:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--workload", a.workload,
               "--size", str(a.size), "--warmup", str(a.warmup), "--runs", str(a.runs), "--max-length", str(a.max_length)]
        cmd += ["--package-root", a.package_root] if a.package_root else []
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print(json.dumps(dict(workload=a.workload, mode=mode, failed=r.returncode)), flush=True)
            return 1  # (nothing more is started on the GPU)
        rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
        timed = [x["device_ms"] for x in rows if not x["warmup"]]
        print(json.dumps(dict(workload=a.workload, mode=mode, median_device_ms=round(statistics.median(timed), 3), min_device_ms=min(timed),
                              max_device_ms=max(timed), median_vcf_ms=round(statistics.median(x["vcf_ms"] for x in rows if not x["warmup"]), 2),
                              runs=len(timed), records=rows[-1]["records"])), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

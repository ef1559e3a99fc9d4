"""A sha256 of everything the query calls return, to compare two builds of the library on the same inputs: every array and
counter of Walks, of Traversals and of Calls (with and without T_INVERSIONS, with T_NESTED, under the profiles
top-level-only, popped and left-normalized, and left-normalized with T_NESTED | T_INVERSIONS), and the VCF text with a fixed
date.  The inputs are those of tools/time_walks.py, time_traversals.py and time_calls.py, then small ones with every query
forced through the second tier, and the traversals once more in a child process with POVU_HIP_TRAV_HASH_BITS=4 (hash
collisions: the exact regrouping).  One line per digest, "<input> <call> <field> <sha256 or number>"; the device times are
left out, so two builds that compute the same print the same.

    python tools/query_digest.py [--package-root <another checkout>] [--scale 1.0]
"""
import argparse
import hashlib
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(package_root):
    """(HipDecomposer, hip module, this tree's workloads): the library of another checkout with --package-root, the inputs
    always this tree's."""
    spec = importlib.util.spec_from_file_location("query_digest_workloads", os.path.join(ROOT, "povu_amd", "workloads.py"))
    w = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = w
    spec.loader.exec_module(w)
    sys.path.insert(0, os.path.abspath(package_root) if package_root else ROOT)
    from povu_amd import HipDecomposer
    from povu_amd import hip
    return HipDecomposer, hip, w


def show(tag, call, r):
    """Every array and every counter of a result, in name order."""
    for k in sorted(vars(r)):
        v = getattr(r, k)
        if k.startswith("_") or k == "device_ms":
            continue
        if isinstance(v, np.ndarray):
            print(tag, call, k, f"{v.dtype}{list(v.shape)}", hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest(), flush=True)
        elif isinstance(v, int):
            print(tag, call, k, v, flush=True)


def show_calls(tag, d, f, H, refs, extra=0):
    for name, flags in (("call", extra), ("call+inv", extra | H.T_INVERSIONS)):
        c = d.call(f, refs, flags=flags)
        show(tag, name, c)
        print(tag, name, "vcf", hashlib.sha256(c.vcf_text(date="20000101").encode()).hexdigest(), flush=True)
        del c


def show_profiles(tag, d, f, H, refs, extra=0):
    """The nested call, the call under every profile, and the left-normalised call with the nested and the inversion records."""
    popped = dict(profile="popped", max_level=0, max_ref_length=64, max_allele_length=64)
    for name, kw in (("call+nested", dict(flags=extra | H.T_NESTED)),
                     ("call/top-level-only", dict(flags=extra, profile="top-level-only")),
                     ("call/popped", dict(flags=extra, **popped)),
                     ("call/left-normalized", dict(flags=extra, profile="left-normalized")),
                     ("call+nested+inv/left-normalized", dict(flags=extra | H.T_NESTED | H.T_INVERSIONS, profile="left-normalized"))):
        c = d.call(f, refs, **kw)
        show(tag, name, c)
        print(tag, name, "vcf", hashlib.sha256(c.vcf_text(date="20000101").encode()).hexdigest(), flush=True)
        del c


def hash_bits_child(a):
    HipDecomposer, H, W = _load(a.package_root)
    d = HipDecomposer(0)
    k = 20000
    d.upload(W.chain_of_bubbles(k))
    f = d.decompose(flags=H.F_NO_STAGE_TIMES)
    d.upload_paths(W.chain_haplotypes(k, 32, seed=1))
    show("chain-hash4", "traversals", d.traversals(f))
    g = W.hprc_shaped([6000, 3000], seed=3, tiny=5)
    d.upload(g)
    f = d.decompose(flags=H.F_NO_STAGE_TIMES)
    d.upload_paths(W.random_walk_paths(g, 32, 6000, seed=4))
    show("hprc-hash4", "traversals", d.traversals(f))
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", help="import povu_amd from this checkout")
    ap.add_argument("--scale", type=float, default=1.0, help="of the timing tools' smaller rows")
    ap.add_argument("--hash-bits-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.hash_bits_child:
        return hash_bits_child(a)
    HipDecomposer, H, W = _load(a.package_root)
    s = a.scale
    d = HipDecomposer(0)

    # ---- walks: the tangled workload and the headline graph at a tenth (tools/time_walks.py)
    for tag, g in (("tangled", W.hprc_tangled(max(1000, int(3e6 * s)), tangle_every=100000, max_tangle=300000)),
                   ("hprc-wg", W.hprc_whole_genome(1e7 * s))):
        d.upload(g)
        f = d.decompose(flags=H.F_NO_STAGE_TIMES)
        show(tag, "walks", d.walks(f))
        del f, g
    g = W.hprc_tangled(30000, tangle_every=10000, max_tangle=3000)
    d.upload(g)
    f = d.decompose(flags=H.F_NO_STAGE_TIMES)
    show("tangled-small", "walks+tier2", d.walks(f, flags=H.W_FORCE_TIER2))
    d.upload_paths(W.random_walk_paths(g, 8, 3000, seed=5))
    show("tangled-small", "traversals", d.traversals(f))
    del f, g

    # ---- traversals (tools/time_traversals.py at a tenth: the tables' smaller rows)
    k = max(100, int(1e7 * s / 3))
    t = max(10, int(2e5 * s))
    for tag, g, paths in (("chain", W.chain_of_bubbles(k), lambda g: W.chain_haplotypes(k, 32, seed=1)),
                          ("towers", W.nested_towers(12, t), lambda g: W.random_walk_paths(g, 32, max(1000, int(2e5 * s)), seed=2)),
                          ("hprc", W.hprc_shaped([max(1000, int(2e5 * s)), max(1000, int(1e5 * s))], seed=3, tiny=5),
                           lambda g: W.random_walk_paths(g, 32, max(1000, int(2e5 * s)), seed=4))):
        d.upload(g)
        f = d.decompose(flags=H.F_NO_STAGE_TIMES)
        d.upload_paths(paths(g))
        show(tag, "traversals", d.traversals(f))
        if tag == "hprc":
            show(tag, "traversals+tier2", d.traversals(f, flags=H.T_FORCE_TIER2))
        del f, g

    # ---- calls (tools/time_calls.py: chain, and an HPRC-shaped graph)
    k = max(100, int(1e6 * s))
    for tag, g, paths in (("call-chain", W.chain_of_bubbles(k), lambda g: W.chain_haplotypes(k, 32, seed=1)),
                          ("call-hprc", W.hprc_shaped([max(1000, int(6e5 * s)), max(1000, int(3e5 * s))], seed=3, tiny=5),
                           lambda g: W.random_walk_paths(g, 32, max(1000, int(6e5 * s)), seed=4))):
        d.upload(g)
        f = d.decompose(flags=H.F_NO_STAGE_TIMES)
        d.upload_paths(W.pansn(paths(g), samples=32))
        d.upload_sequences(W.random_sequences(g, 5, max_len=300))
        show_calls(tag, d, f, H, ["sample0#"])
        if tag == "call-hprc":
            show_calls(tag + "+tier2", d, f, H, ["sample0#"], extra=H.T_FORCE_TIER2)
        del f, g

    # ---- inversions (tools/time_calls.py: inverted, and the same with every haplotype forward)
    k = max(100, int(1e8 * 0.01 * s / 3))
    g = W.chain_of_bubbles(k)
    base = W.chain_haplotypes(k, 32, seed=1, reverse_every=0)
    cut = lambda j: (base.ids[int(base.off[j]):int(base.off[j + 1])], base.rev[int(base.off[j]):int(base.off[j + 1])])  # noqa: E731
    copied = W._paths(base.names, [cut(0 if 1 <= j <= 4 else j) for j in range(32)])
    d.upload(g)
    f = d.decompose(flags=H.F_NO_STAGE_TIMES)
    d.upload_sequences(W.random_sequences(g, 1, max_len=30))
    for tag, p in (("inv-forward", W.pansn(base, samples=32)),
                   ("inv-inverted", W.pansn(W.inverted_haplotypes(copied, 1000, 2, 2000, 2, keep=(0,)), samples=32))):
        d.upload_paths(p)
        show_calls(tag, d, f, H, ["sample0#"])
    show_calls("inv-inverted+tier2", d, f, H, ["sample0#"], extra=H.T_FORCE_TIER2)
    del f, g

    # ---- nested calls and profiles (tools/time_calls.py: skip and tandem at a tenth, the tandem haplotypes with intervals walked
    # backwards so that the last call has every family of blocks), then small ones through the second tier
    size = len(W._skip_template(2, 2)[0])
    for tag, units, haps, extra in (("skip", max(4, int(1e5 * s / size)), 64, 0), ("skip-small+tier2", 40, 16, H.T_FORCE_TIER2)):
        g = W.skip_nested(units, 2)
        d.upload(g)
        f = d.decompose(flags=H.F_NO_STAGE_TIMES)
        d.upload_paths(W.skip_haplotypes(units, 2, haps, seed=1))
        d.upload_sequences(W.random_sequences(g, 5, max_len=16))
        show_profiles(tag, d, f, H, ["hap0#", "hap3#"], extra=extra)
        del f, g
    for tag, units, extra in (("tandem", max(20, int(1e4 * s)), 0), ("tandem-small+tier2", 200, H.T_FORCE_TIER2)):
        g, seqs = W.tandem_indels(units, 1)
        d.upload(g)
        f = d.decompose(flags=H.F_NO_STAGE_TIMES)
        d.upload_paths(W.inverted_haplotypes(W.tandem_haplotypes(units, 1, 8), max(4, units // 10), 3, 9, seed=4, keep=(0,)))
        d.upload_sequences(seqs)
        show_profiles(tag, d, f, H, ["hap0#", "hap3#"], extra=extra)
        del f, g
    d.close()

    # ---- hash collisions: a process of its own (the hook is read from the environment)
    cmd = [sys.executable, os.path.abspath(__file__), "--hash-bits-child"] + (["--package-root", a.package_root] if a.package_root else [])
    sys.stdout.flush()
    subprocess.check_call(cmd, env=dict(os.environ, POVU_HIP_TRAV_HASH_BITS="4"))


if __name__ == "__main__":
    main()

"""GPU nested calls (povu_hip_call with POVU_HIP_T_NESTED, povu_hip_call_profile, `povu call --nested --profile`) against
the plain-Python restatement (tests/nested_ref.py), array for array and VCF text for VCF text: skip_nested graphs of depth
0, 1 and 3 with PanSN haplotypes, nested_towers and hprc_shaped with random-walk and noise paths, a -s forest, two
reference prefixes over two components, the forced tier-2 kernels, a narrowed hash in a child process, the three
profiles, the reference's fixture through the CLI and gfa2vcf, the plain call left as it was, and
the wide cohort of 131 samples in 261 slots (tests/cohort_cases.py)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cohort_cases as CC
import nested_ref as N
import vcf_ref as V
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
DATE = "00000000"
NIL = 0xFFFFFFFF
FIXTURE = "downstream_repetitive/popped-parent-child-rescue"


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _flags(r):
    return ((H.CALL_ANCHORED if r["anchored"] else 0) | (H.CALL_TANGLED if r["tangled"] else 0) |
            (H.CALL_INS if r["vartype"] == "INS" else 0) | (H.CALL_DEL if r["vartype"] == "DEL" else 0) |
            (H.CALL_COLLAPSED if r["collapsed"] else 0) | (H.CALL_RESCUED if r["rescued"] else 0))


def _same(c, want, counters):
    """The device's arrays equal the restatement's records."""
    assert c.nested and c.n_records == len(want)
    assert [(int(c.path[i]), int(c.pos[i]), int(c.query[i]), int(c.first[i])) for i in range(c.n_records)] == \
        [(r["path"], r["pos"], r["q"], r["first"]) for r in want]
    assert c.n_alleles.tolist() == [r["n_classes"] for r in want]
    assert c.ref_allele.tolist() == [r["ref_class"] for r in want]
    assert c.gt.tolist() == [[H.GT_MISSING if g is None else g for g in r["slots"]] for r in want]
    assert c.ac.tolist() == [x for r in want for x in r["ac"]]
    assert c.an.tolist() == [r["an"] for r in want] and c.ns.tolist() == [r["ns"] for r in want]
    assert c.level.astype(np.int32).tolist() == [r["lv"] for r in want]
    assert c.parent_query.tolist() == [NIL if r["parent"] is None else r["parent"] for r in want]
    assert c.flags.tolist() == [_flags(r) for r in want]
    assert dict(n_enclosed=c.n_enclosed, n_collapsed_sites=c.n_collapsed_sites, n_popped=c.n_popped, n_rescued=c.n_rescued) == counters
    # REF is spelled on its own exactly where it is not its class's representative
    own = [int(c.ref_spelled[i]) != int(c.block_off[c.block[i]]) + int(c.ref_allele[i]) for i in range(c.n_records)]
    assert own == [not r["ref_is_rep"] for r in want]


def _setup(d, g, paths, flags=0, seed=1, max_len=300):
    d.upload(g)
    f = d.decompose(flags=flags)
    d.upload_paths(paths)
    seqs = W.random_sequences(g, seed, max_len=max_len)
    d.upload_sequences(seqs)
    steps = [paths.steps(k) for k in range(len(paths))]
    sq = dict(zip(g.vid.tolist(), seqs))
    sites = V.sites_of_pvst([f.text(i) for i in range(len(f))])
    return f, sites, steps, sq


def _check(d, g, paths, prefixes, flags=0, tflags=0, seed=1, max_len=300, profile=None, setup=None, **popt):
    f, sites, steps, sq = setup or _setup(d, g, paths, flags, seed, max_len)
    names = list(paths.names)
    c = d.call(f, prefixes, flags=tflags | H.T_NESTED, profile=profile, **popt)
    want, counters = N.call_full(sites, names, steps, sq, prefixes, profile=profile, **popt)
    _same(c, want, counters)
    assert c.vcf_text(date=DATE) == N.vcf_text(names, steps, sq, want, prefixes, date=DATE, profile=profile)
    return c, want, counters


def _skip(units, depth, haps, seed):
    g = W.skip_nested(units, depth, seed)
    p = W.skip_haplotypes(units, depth, haps, seed)
    return g, W.pansn(p, samples=(haps + 1) // 2)


@pytest.mark.parametrize("units,depth,haps", [(40, 0, 8), (30, 1, 8), (8, 3, 16)])
def test_skip_nested(hip, units, depth, haps):
    g, p = _skip(units, depth, haps, seed=depth + 1)
    setup = _setup(hip, g, p, seed=depth + 1, max_len=12)
    c, want, counters = _check(hip, g, p, ["sample0#1"], setup=setup)
    # what keeps this from passing vacuously, on the restatement's answer
    with_records = {r["q"] for r in want}
    assert len(with_records) >= 10 and 5 * len({r["q"] for r in want if r["collapsed"]}) >= len(with_records)
    assert counters["n_enclosed"] > 0
    if depth == 3:
        assert max(r["lv"] for r in want) >= 2
    # the wave kernels alone give the same
    c2, _, _ = _check(hip, g, p, ["sample0#1"], tflags=H.T_FORCE_TIER2, setup=setup)
    assert c2.vcf_text(date=DATE) == c.vcf_text(date=DATE)
    # the profiles
    raw_bytes = c.n_seq_bytes
    _check(hip, g, p, ["sample0#1"], setup=setup, profile="raw-graph")
    _, top, _ = _check(hip, g, p, ["sample0#1"], setup=setup, profile="top-level-only")
    assert top and len(top) < len(want)
    cp, popped, counters = _check(hip, g, p, ["sample0#1"], setup=setup, profile="popped", max_level=0, max_ref_length=8,
                                  max_allele_length=8)
    assert counters["n_popped"] >= 1 and counters["n_rescued"] >= 1
    assert cp.n_seq_bytes < raw_bytes  # (the popped records were never spelled)
    _check(hip, g, p, ["sample0#1"], setup=setup, profile="popped", max_level=1, max_ref_length=20, tflags=H.T_FORCE_TIER2)
    # two references: some REF is not its class's representative
    c3, want3, _ = _check(hip, g, p, ["sample0#1", "sample1#2"], setup=setup)
    assert any(not r["ref_is_rep"] for r in want3)


@pytest.mark.parametrize("ref", CC.REFS)
def test_wide_cohort(hip, ref):
    """131 samples, 261 slots (tests/cohort_cases.py): three rounds of the lane-per-sample loop under T_NESTED, plain and popped."""
    g, p = CC.wide_chain()
    setup = _setup(hip, g, p, seed=CC.SEQ_SEED, max_len=CC.MAX_LEN)
    c, want, _ = _check(hip, g, p, [ref], setup=setup)
    assert c.n_slots == 261 and len(want) == 12 and {r["ns"] for r in want} == {129, 130, 131}
    _check(hip, g, p, [ref], setup=setup, tflags=H.T_FORCE_TIER2)
    _check(hip, g, p, [ref], setup=setup, profile="popped", max_level=0, max_ref_length=2, max_allele_length=2)


def test_long_alleles_take_the_wave_tier(hip):
    # depth 3 units are 150 steps long: their alleles are beyond tier 1's 64 steps without any flag
    g, p = _skip(6, 3, 12, seed=9)
    _, want, _ = _check(hip, g, p, ["sample0#1"], seed=9, max_len=5)
    assert any(r["last"] - r["first"] + 1 > 64 and r["collapsed"] for r in want)


def test_nested_towers_and_hprc_random_walks(hip):
    g = W.nested_towers(4, 30)
    p = W.random_walk_paths(g, 12, 400, seed=3)
    _check(hip, g, W.pansn(p, samples=4), ["sample0#1", "sample2#2"], seed=3)
    g = W.hprc_shaped([500, 300], seed=9, tiny=3)
    rw = W.random_walk_paths(g, 10, 800, seed=4)
    nz = W.noise_paths(g, 4, 300, seed=5)
    both = W.Paths(list(rw.names) + list(nz.names), np.concatenate([rw.off, rw.off[-1] + nz.off[1:]]),
                   np.concatenate([rw.ids, nz.ids]), np.concatenate([rw.rev, nz.rev]))
    setup = _setup(hip, g, both, seed=4)
    _check(hip, g, both, ["walk0", "walk3"], setup=setup)
    _check(hip, g, both, ["walk0", "walk3"], setup=setup, profile="popped", max_ref_length=50, tflags=H.T_FORCE_TIER2)


def test_subflubble_forest_and_two_components(hip):
    g = W.bubble_zoo(6, 8, 2)
    p = W.random_walk_paths(g, 10, 300, seed=7)
    _check(hip, g, W.pansn(p, samples=5), ["sample0#1"], flags=H.F_SUBFLUBBLES, seed=7)
    g = W.hprc_shaped([300, 200], seed=11)
    p = W.random_walk_paths(g, 16, 600, seed=8)
    c, want, _ = _check(hip, g, W.pansn(p, samples=4), ["sample0#", "sample3#2"], seed=8)
    assert len({r["path"] for r in want}) >= 2


def test_flag_off_is_the_plain_call(hip):
    g, p = _skip(30, 1, 8, seed=2)
    f, sites, steps, sq = _setup(hip, g, p, seed=2, max_len=12)
    names = list(p.names)
    plain = hip.call(f, ["sample0#1"])
    want = V.call(sites, names, steps, sq, ["sample0#1"])
    assert not plain.nested and plain.n_records == len(want)
    assert plain.vcf_text(date=DATE) == V.vcf_text(names, steps, sq, want, ["sample0#1"], date=DATE)
    assert plain.level.astype(np.int32).tolist() == [r["lv"] for r in want] and set(plain.parent_query.tolist()) <= {NIL}
    assert plain.ref_spelled.tolist() == [int(plain.block_off[plain.block[i]]) + int(plain.ref_allele[i]) for i in range(len(want))]
    assert (plain.n_enclosed, plain.n_collapsed_sites, plain.n_popped, plain.n_rescued) == (0, 0, 0, 0)
    assert plain.n_alleles.tolist() == [1 + len(r["alts"]) for r in want]
    assert plain.gt.tolist() == [[H.GT_MISSING if x is None else x for x in r["slots"]] for r in want]
    # raw-graph as a profile without the flag is the plain call too; the nested one differs on this input
    same = hip.call(f, ["sample0#1"], profile="raw-graph")
    assert same.vcf_text(date=DATE) == plain.vcf_text(date=DATE)
    nested = hip.call(f, ["sample0#1"], flags=H.T_NESTED)
    assert nested.vcf_text(date=DATE) != plain.vcf_text(date=DATE) and nested.n_seq_bytes < plain.n_seq_bytes
    with pytest.raises(ValueError):
        hip.call(f, ["sample0#1"], profile="flat")
    # inversion records pass a profile unchanged
    inv = W.inverted_haplotypes(p, 6, 3, 9, seed=4, keep=(0,))
    hip.upload_paths(inv)
    a = hip.call(f, ["sample0#1"], flags=H.T_INVERSIONS)
    b = hip.call(f, ["sample0#1"], flags=H.T_INVERSIONS, profile="top-level-only")
    subr = lambda c: [ln for ln in c.vcf_text(date=DATE).splitlines() if "VARTYPE=SUBR" in ln]  # noqa: E731
    assert a.n_inv_records > 0 and subr(a) == subr(b)
    assert all(ln.split("\t")[2].endswith(":top") for ln in b.vcf_text(date=DATE).splitlines()
               if not ln.startswith("#") and "VARTYPE=SUBR" not in ln)


def _digest(c):
    h = hashlib.sha256()
    for k in ("query", "path", "first", "ref_allele", "n_alleles", "an", "ns", "level", "parent_query", "flags", "ac", "gt", "pos"):
        h.update(np.ascontiguousarray(getattr(c, k)).tobytes())
    h.update(c.vcf_text(date=DATE).encode())
    return h.hexdigest()


def _hash_case():
    return _skip(12, 2, 24, seed=5)


def child_narrow_hash():
    """Run in a child process under POVU_HIP_TRAV_HASH_BITS=4: the nested call against the restatement, its digest printed."""
    d = HipDecomposer(0)
    g, p = _hash_case()
    setup = _setup(d, g, p, seed=5, max_len=6)
    assert d.traversals(setup[0]).n_hash_splits > 0  # (the hook is in force: sixteen hash values collide)
    c, _, _ = _check(d, g, p, ["sample0#1"], setup=setup)
    c2, _, _ = _check(d, g, p, ["sample0#1"], setup=setup, tflags=H.T_FORCE_TIER2)
    print("DIGEST", _digest(c), _digest(c2))
    d.close()


def test_narrow_hash_does_not_change_the_answer(hip):
    g, p = _hash_case()
    c, want, _ = _check(hip, g, p, ["sample0#1"], seed=5, max_len=6)
    assert max(r["n_classes"] for r in want) >= 3
    env = dict(os.environ, POVU_HIP_TRAV_HASH_BITS="4",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_nested as T; T.child_narrow_hash()"], capture_output=True, text=True,
                       timeout=600, env=env, cwd=os.path.join(ROOT, "tests"))
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0].split()
    assert line[1] == line[2] == _digest(c)


# ---- the CLI

def _rows(text):
    out = []
    for ln in text.splitlines():
        if ln and not ln.startswith("#"):
            f = ln.split("\t")
            info = dict(kv.split("=", 1) for kv in f[7].split(";"))
            out.append(dict(chrom=f[0], pos=int(f[1]), id=f[2], ref=f[3], alts=f[4].split(","), ac=[int(x) for x in info["AC"].split(",")],
                            af=[float(x) for x in info["AF"].split(",")], an=int(info["AN"]), ns=int(info["NS"]), at=info["AT"].split(","),
                            vartype=info["VARTYPE"], tangled=info["TANGLED"], es=info["ES"], lv=int(info["LV"]), gt=f[9:],
                            info={k: v for k, v in info.items() if k in N._DESC}))
    return out


def test_fixture_through_the_cli_and_gfa2vcf(golden_dir, tmp_path):
    want = json.load(open(os.path.join(golden_dir, "reference_nested_records.json")))
    gfa = os.path.join(golden_dir, "gfa", FIXTURE + ".gfa")
    out = tmp_path / "forest"
    out.mkdir()
    r = subprocess.run([POVU, "decompose", "-i", gfa, "-o", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names, paths, seqs = V.read_gfa(gfa)
    sites = V.sites_of_pvst([(out / "1.pvst").read_text()])
    popt = want["popped_options"]
    for profile, rows in sorted(want["profiles"].items()):
        extra = ["--max-level", str(popt["max_level"]), "--max-ref-length=" + str(popt["max_ref_length"]), "--max-allele-length",
                 str(popt["max_allele_length"])] if profile == "popped" else []
        cmds = [[POVU, "call", "-i", gfa, "-f", str(out), "-P", "HG1", "--nested", "--profile", profile] + extra,
                [POVU, "gfa2vcf", "-i", gfa, "-P", "HG1", "--stdout", "--nested", "--profile=" + profile] + extra]  # (raw-graph does not imply --nested)
        ref = N.call(sites, names, paths, seqs, ["HG1"], profile=profile, **(popt if profile == "popped" else {}))
        for cmd in cmds:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, POVU_CALL_EXE=POVU))
            assert r.returncode == 0, r.stderr
            got = _rows(r.stdout)
            assert len(got) == len(rows)
            for g, w in zip(got, rows):
                for k in g:
                    if k == "af":
                        assert all(abs(a - b) <= 0.05 for a, b in zip(g[k], w[k]))
                    elif k == "pos" and w["es"] == ">2>4":
                        assert (g[k], w[k]) == (4, 3)  # (tests/test_nested_ref.py says why)
                    else:
                        assert g[k] == w[k], (profile, k)
            assert r.stdout.split("\n", 2)[2] == N.vcf_text(names, paths, seqs, ref, ["HG1"], date=DATE, profile=profile).split("\n", 2)[2]
    # without --nested the call is the plain one; refusals
    r = subprocess.run([POVU, "call", "-i", gfa, "-f", str(out), "-P", "HG1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split("\n", 2)[2] == V.vcf_text(names, paths, seqs, V.call(sites, names, paths, seqs, ["HG1"]),
                                                                            ["HG1"], date=DATE).split("\n", 2)[2]
    r = subprocess.run([POVU, "call", "-i", gfa, "-f", str(out), "-P", "HG1", "--profile", "flat"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--profile" in r.stderr
    r = subprocess.run([POVU, "call", "-i", gfa, "-f", str(out), "-P", "HG1", "--max-level", "x"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--max-level" in r.stderr
    r = subprocess.run([POVU, "call", "-i", gfa, "-f", str(out), "-P", "HG1", "--nested", "--gpus", "2"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1

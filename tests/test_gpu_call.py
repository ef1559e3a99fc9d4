"""GPU variant calls (povu_hip_call, `povu call`) against the plain-Python restatement (tests/vcf_ref.py), array for array
and VCF text for VCF text, on every graph family with PanSN haplotypes, random-walk and noise paths, reversed references,
-s forests, several reference prefixes over two components, a graph of more than 10^5 segments and the forced tier-2 scans;
the ten flubble fixtures through `povu decompose` and `povu call` against the records the reference states for them;
gfa2vcf end to end; the refusals; two graphs in one context; the wide cohort of 131 samples in 261 slots (tests/cohort_cases.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import call_modes_cases as MC
import cohort_cases as CC
import vcf_ref as V
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
DATE = "00000000"


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _check(d, g, paths, prefixes, flags=0, tflags=0, seed=1, max_len=300):
    d.upload(g)
    f = d.decompose(flags=flags)
    d.upload_paths(paths)
    seqs = W.random_sequences(g, seed, max_len=max_len)
    d.upload_sequences(seqs)
    c = d.call(f, prefixes, flags=tflags)
    steps = [paths.steps(k) for k in range(len(paths))]
    sq = dict(zip(g.vid.tolist(), seqs))
    # the yardstick's own sites, from the forest's PVST texts; the library's sites (povu_hip_forest_sites) equal them
    sites = V.sites_of_pvst([f.text(i) for i in range(len(f))])
    got = f.sites()
    assert got.n == len(sites)
    for k, col in (("id1", [s["s"][0] for s in sites]), ("or1", [s["s"][1] for s in sites]), ("id2", [s["z"][0] for s in sites]),
                   ("or2", [s["z"][1] for s in sites]), ("parent", [s["parent"] & 0xFFFFFFFF for s in sites]),
                   ("height", [s["height"] for s in sites]), ("family", [ord(s["fam"]) for s in sites]),
                   ("tree", [s["tree"] for s in sites])):
        assert getattr(got, k).tolist() == col, k
    want = V.call(sites, list(paths.names), steps, sq, prefixes)
    assert c.n_records == len(want)
    assert [(int(c.path[i]), int(c.pos[i]), int(c.query[i]), int(c.first[i])) for i in range(c.n_records)] == \
        [(r["path"], r["pos"], r["q"], r["first"]) for r in want]
    for i, r in enumerate(want):
        a0, a1 = int(c.ac_off[i]), int(c.ac_off[i + 1])
        assert [int(x) for x in c.ac[a0:a1]] == r["ac"] and int(c.an[i]) == r["an"] and int(c.ns[i]) == r["ns"], i
    got = c.vcf_text(date=DATE)
    assert got == V.vcf_text(list(paths.names), steps, sq, want, prefixes, date=DATE)
    return c, want


def _kinds(want):
    return {r["vartype"] for r in want}, {len(r["alts"]) > 1 for r in want}


def test_chain_of_bubbles_haplotypes(hip):
    g = W.chain_of_bubbles(300)
    p = W.pansn(W.chain_haplotypes(300, 16, seed=5), samples=8)
    c, want = _check(hip, g, p, ["sample0#1"])
    assert len(want) > 100 and {"INS", "DEL"} <= _kinds(want)[0]  # (every unit has the a > b skip: no SUB)
    assert c.n_seq_bytes > 0 and c.device_ms > 0
    # a reversed reference (every fourth haplotype is written '<')
    _check(hip, g, p, ["sample1#2"], seed=2)


def test_nested_towers_and_hprc_random_walks(hip):
    g = W.nested_towers(4, 30)
    p = W.random_walk_paths(g, 12, 400, seed=3)
    _check(hip, g, W.pansn(p, samples=4), ["sample0#1", "sample2#2"], seed=3)
    g = W.hprc_shaped([500, 300], seed=9, tiny=3)
    rw = W.random_walk_paths(g, 10, 800, seed=4)
    nz = W.noise_paths(g, 4, 300, seed=5)
    both = W.Paths(list(rw.names) + list(nz.names), np.concatenate([rw.off, rw.off[-1] + nz.off[1:]]),
                   np.concatenate([rw.ids, nz.ids]), np.concatenate([rw.rev, nz.rev]))
    _check(hip, g, both, ["walk0", "walk3"], seed=4)


def test_subflubble_forest(hip):
    g = W.bubble_zoo(6, 8, 2)
    p = W.random_walk_paths(g, 10, 300, seed=7)
    _check(hip, g, W.pansn(p, samples=5), ["sample0#1"], flags=H.F_SUBFLUBBLES, seed=7)
    # the T / O relabelling alone: those vertices are skipped like subflubbles
    _check(hip, g, W.pansn(p, samples=5), ["sample0#1"], flags=H.F_LEAF_SUBFLUBBLES, seed=7)


def test_references_on_two_components(hip):
    g = W.hprc_shaped([300, 200], seed=11)
    p = W.random_walk_paths(g, 16, 600, seed=8)
    c, want = _check(hip, g, W.pansn(p, samples=4), ["sample0#", "sample3#2"], seed=8)
    assert len({r["path"] for r in want}) >= 2


def test_large_graph_and_tier2(hip):
    g = W.chain_of_bubbles(40000)  # 1.2 * 10^5 segments
    p = W.pansn(W.chain_haplotypes(40000, 6, seed=13), samples=3)
    c, want = _check(hip, g, p, ["sample0#1"], seed=13, max_len=40)
    assert c.n_records > 10000
    g = W.chain_of_bubbles(400)
    _check(hip, g, W.pansn(W.chain_haplotypes(400, 8, seed=14), samples=4), ["sample0#1"], tflags=H.T_FORCE_TIER2, seed=14)


@pytest.mark.parametrize("ref", CC.REFS)
def test_wide_cohort(hip, ref):
    """131 samples, 261 slots (tests/cohort_cases.py): the lane-per-sample loop of the record kernel takes three rounds, the
    reference's slot in the first or in the last; GT by its array as well as by the text."""
    g, p = CC.wide_chain()
    for tflags in (0, H.T_FORCE_TIER2):
        c, want = _check(hip, g, p, [ref], tflags=tflags, seed=CC.SEQ_SEED, max_len=CC.MAX_LEN)
        assert len(c.samples) == 131 and c.n_slots == 261 and c.n_records == 12
        assert c.gt.tolist() == [[H.GT_MISSING if v is None else v for v in r["slots"]] for r in want]
        assert [bool(x & H.CALL_TANGLED) for x in c.flags.tolist()] == [r["tangled"] for r in want]
        assert sum(r["tangled"] for r in want) == 4 and {r["ns"] for r in want} == {129, 130, 131}


def test_refusals_and_two_graphs(hip):
    g = W.chain_of_bubbles(20)
    hip.upload(g)
    f = hip.decompose()
    p = W.pansn(W.chain_haplotypes(20, 4, seed=1), samples=2)
    hip.upload_paths(p)
    with pytest.raises(RuntimeError, match="no sequences"):
        hip.call(f, ["sample0"])
    seqs = W.random_sequences(g, 1)
    with pytest.raises(RuntimeError, match="'\\*'"):
        hip.upload_sequences(["*"] * g.n_vtx)
    with pytest.raises(RuntimeError, match="segments"):
        hip.upload_sequences(seqs[:-1])
    hip.upload_sequences(["ACGT"] * g.n_vtx)
    with pytest.raises(RuntimeError, match="no path name"):
        hip.call(f, ["nobody"])
    hip.upload_sequences(["AQ"] * g.n_vtx)
    with pytest.raises(RuntimeError, match="segment \\d+ holds a byte"):
        hip.call(f, ["sample0"])
    hip.upload_sequences(seqs)
    assert hip.call(f, ["sample0"]).n_records > 0
    # a second graph drops the sequences (and the paths)
    g2 = W.chain_of_bubbles(30)
    hip.upload(g2)
    f2 = hip.decompose()
    hip.upload_paths(W.pansn(W.chain_haplotypes(30, 4, seed=2), samples=2))
    with pytest.raises(RuntimeError, match="no sequences"):
        hip.call(f2, ["sample0"])


def test_which_modes_combine():
    """Every pair of modes and every (mode, profile) on the worked example of the clustered calls (six segments): the call is
    refused exactly where the recorded answers say so (tests/golden/call_modes.json, which tests/test_call_modes.py holds the
    table of call_modes.hpp to), with the recorded library text, and `povu call` refuses the same requests.  A refused call
    returns before it takes any device memory (the arenas of a context that has made no call stay as they were, so no kernel
    had anything to run on); an accepted one runs."""
    d = HipDecomposer(0)
    try:
        f = MC.resident_example(d)
        before = d.arenas()
        accepted = []
        for modes, profile in MC.REQUESTS:
            lib, cli = MC.expected(modes, profile)
            assert MC.cli_answer(modes, profile) == cli and bool(lib) == bool(cli), (modes, profile)
            if not lib:
                accepted.append((modes, profile))
                continue
            with pytest.raises(RuntimeError) as e:
                d.call(f, ["HG1"], **MC.library_kwargs(modes, profile))
            assert str(e.value) == lib, (modes, profile)
        assert d.arenas() == before and len(accepted) > 10 and len(accepted) < len(MC.REQUESTS) - 10
        for modes, profile in accepted:
            c = d.call(f, ["HG1"], **MC.library_kwargs(modes, profile))
            assert c.device_ms > 0 and c.vcf_text(date=DATE).startswith("##fileformat=VCFv4.2\n##fileDate=" + DATE), (modes, profile)
        assert d.arenas() != before  # (a call that runs does take its arenas: the comparison above can tell)
    finally:
        d.close()


# ---- the CLI

def _golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "reference_vcf_records.json")))


def _parse_vcf(text):
    samples, recs = None, []
    for ln in text.splitlines():
        if ln.startswith("#CHROM"):
            samples = ln.split("\t")[9:]
        elif ln and not ln.startswith("#"):
            f = ln.split("\t")
            info = dict(kv.split("=", 1) for kv in f[7].split(";"))
            recs.append(dict(chrom=f[0], pos=int(f[1]), id=f[2], ref=f[3], alts=f[4].split(","), at=info["AT"].split(","),
                             vartype=info["VARTYPE"], lv=int(info["LV"]), gt=f[9:], ac=[int(x) for x in info["AC"].split(",")],
                             an=int(info["AN"])))
    return samples, recs


def test_fixtures_through_the_cli(golden_dir, tmp_path):
    want = _golden(golden_dir)
    for name, fx in sorted(want["fixtures"].items()):
        gfa = os.path.join(golden_dir, "gfa", name + ".gfa")
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([POVU, "decompose", "-i", gfa, "-o", str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([POVU, "call", "-i", gfa, "-f", str(out), "-P", want["reference_prefix"]], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        samples, recs = _parse_vcf(r.stdout)
        assert samples == fx["samples"] and recs == fx["records"], name
        # the same text as the restatement, date masked
        names, paths, seqs = V.read_gfa(gfa)
        sites = V.sites_of_pvst([(out / "1.pvst").read_text()])
        ref = V.vcf_text(names, paths, seqs, V.call(sites, names, paths, seqs, ["HG1"]), ["HG1"], date=DATE)
        assert r.stdout.split("\n", 2)[2] == ref.split("\n", 2)[2]


def test_gfa2vcf_end_to_end(golden_dir):
    gfa = os.path.join(golden_dir, "gfa", "nested_deletion.gfa")
    r = subprocess.run([POVU, "gfa2vcf", "-i", gfa, "-P", "HG1", "--stdout"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, POVU_CALL_EXE=POVU))
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if not ln.startswith("#")]
    assert lines == ["HG1#1#chr1\t2\t>1>4\tCT\tC\t60\tPASS\tAC=1;AF=0.5;AN=2;NS=2;AT=>1>3,>1;VARTYPE=DEL;TANGLED=F;ES=>1>4;"
                     "LV=1\tGT\t0\t1\t."]


def test_split_files_and_cli_refusals(tmp_path):
    g = W.hprc_shaped([200, 150], seed=21)
    p = W.pansn(W.random_walk_paths(g, 8, 400, seed=22), samples=4)
    seqs = W.random_sequences(g, 23, max_len=30, empty=0.0)  # (a GFA S line needs a sequence)
    gfa = tmp_path / "g.gfa"
    gfa.write_text(g.to_gfa(seqs) + p.to_gfa())
    forest = tmp_path / "forest"
    forest.mkdir()
    r = subprocess.run([POVU, "decompose", "-i", str(gfa), "-o", str(forest)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    outdir = tmp_path / "vcf"
    r = subprocess.run([POVU, "-t", "4", "call", "-i", str(gfa), "-f", str(forest), "-P", "sample0#", "-P", "sample1#", "-o",
                        str(outdir)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    texts = {k: (outdir / f"{k}.vcf").read_text() for k in ("sample0#", "sample1#")}
    r = subprocess.run([POVU, "call", "-i", str(gfa), "-f", str(forest), "sample0#", "sample1#"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    names = list(p.names)
    steps = [p.steps(k) for k in range(len(p))]
    sq = dict(zip(g.vid.tolist(), seqs))
    pv = sorted(forest.glob("*.pvst"), key=lambda x: int(x.stem))
    recs = V.call(V.sites_of_pvst([x.read_text() for x in pv]), names, steps, sq, ["sample0#", "sample1#"])
    mask = lambda t: t.split("\n", 2)[2]  # noqa: E731
    assert mask(r.stdout) == mask(V.vcf_text(names, steps, sq, recs, ["sample0#", "sample1#"], date=DATE))
    for k, t in texts.items():
        assert mask(t) == mask(V.vcf_text(names, steps, sq, recs, ["sample0#", "sample1#"], date=DATE, only=k))
    # refusals: no matching path, a '*' sequence, a non-IUPAC byte, PVSTs of another graph
    r = subprocess.run([POVU, "call", "-i", str(gfa), "-f", str(forest), "-P", "nobody"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "nobody" in r.stderr
    star = tmp_path / "star.gfa"
    star.write_text(g.to_gfa(["*"] + seqs[1:]) + p.to_gfa())
    r = subprocess.run([POVU, "call", "-i", str(star), "-f", str(forest), "-P", "sample0#"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "'*'" in r.stderr
    bad = tmp_path / "bad.gfa"
    bad.write_text(g.to_gfa(["AQA"] * g.n_vtx) + p.to_gfa())
    r = subprocess.run([POVU, "call", "-i", str(bad), "-f", str(forest), "-P", "sample0#"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "holds a byte" in r.stderr
    other = W.chain_of_bubbles(10)
    og = tmp_path / "other.gfa"
    op = W.pansn(W.chain_haplotypes(10, 2, seed=1), samples=1)
    og.write_text(other.to_gfa() + op.to_gfa())
    r = subprocess.run([POVU, "call", "-i", str(og), "-f", str(forest), "-P", "sample0#"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "segment" in r.stderr

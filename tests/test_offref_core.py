"""The rules of the off-reference calls as the device runs them (povu_amd/csrc/hip/offref_rules.hpp), on the CPU: `offref_check`
(povu_amd/csrc/host/offref_check.cpp, built with -fsanitize=address,undefined) against the restatement (tests/offref_ref.py)
on the hand cases, the fixture and random small forests and intervals.  No GPU."""
import os
import random
import subprocess

import pytest

import offref_cases as OC
import offref_ref as F
import traversals_ref as TR
import vcf_ref as V

ROOT = OC.ROOT


@pytest.fixture(scope="module")
def offref_check():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "povu_amd", "csrc"), "offref_check", "-s"])
    return os.path.join(ROOT, "build", "obj", "offref_check")


def run(exe, blocks):
    """The program's lines for the blocks; it must end clean under the sanitizers."""
    r = subprocess.run([exe], input="\n".join(blocks) + "\n", capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and not r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "offref_check: ok"
    return lines[:-1]


def sites_block(sites, callable_, travs):
    return "\n".join([f"sites {len(sites)}"] + [f"{s['parent']} {s['fam']} {int(c)} {len(t)}" for s, c, t in zip(sites, callable_, travs)])


def states(sites, names, paths, prefixes):
    index = TR.PathIndex(paths)
    travs = [TR.traversals_of(index, s["s"], s["z"])[1] for s in sites]
    refs = V.ref_paths(names, prefixes)
    return travs, F.site_states(sites, {r: index.paths[r] for r in refs}, travs)


def test_hand_cases_and_fixture(offref_check, tmp_path):
    graphs = [OC.gfa_of(n) for n in sorted(OC.golden()["cases"])] + [OC.FIXTURE]
    n_hosted = 0
    for k, gfa in enumerate(graphs):
        sites, names, paths, seqs, _ = OC.load(gfa, tmp_path / str(k))
        travs, (callable_, called, cand, off, _sur) = states(sites, names, paths, ["HG1"])
        got = run(offref_check, [sites_block(sites, callable_, travs)])
        assert got == [f"{int(c)} {int(o)}" for c, o in zip(cand, off)], gfa
        recs, _ = F.call(sites, names, paths, seqs, ["HG1"])
        alleles = [len({t[4] for t in tv}) for tv in travs]
        for r in (r for r in recs if r["offref"]):
            last = next(t[2] for t in travs[r["q"]] if t[0] == r["path"] and t[1] == r["first"])
            hosts = [(t[1], t[2], q) for q in range(len(sites)) if called[q] and alleles[q] >= 2 for t in travs[q] if t[0] == r["path"]]
            got = run(offref_check, ["\n".join([f"hosts {r['first']} {last} {len(hosts)}"] + ["%d %d %d" % h for h in hosts])])
            assert got == [f"{-1 if r['host'] is None else r['host']} " + ("-1" if r["host"] is None else got[0].split()[1])], gfa
            n_hosted += r["host"] is not None
    assert n_hosted >= 5


def test_random_forests_and_intervals(offref_check):
    rng = random.Random(7)
    blocks, want = [], []
    for _ in range(200):
        n = rng.randint(1, 12)
        sites = [dict(parent=rng.randint(-1, q - 1) if q else -1, fam=rng.choice("FFFFFTOCMS"), tree=0, s=(0, 0), z=(1, 0)) for q in range(n)]
        callable_ = [rng.random() < 0.4 for _ in range(n)]
        travs = [[(0, 0, 1, 0, 0)] * rng.randint(0, 2) for _ in range(n)]
        # the restatement's rule on its own (site_states derives callable from paths; here it is given)
        skip = [False] * n
        for q in range(n):
            skip[q] = sites[q]["fam"] in V.SUBFLUBBLE or (sites[q]["parent"] >= 0 and skip[sites[q]["parent"]])
        callable_ = [c and not sk for c, sk in zip(callable_, skip)]
        cand = [not skip[q] and not callable_[q] and len(travs[q]) > 0 for q in range(n)]
        off = list(cand)
        for q in range(n):
            if sites[q]["parent"] >= 0 and (callable_[q] or cand[q]):
                off[sites[q]["parent"]] = False
        blocks.append(sites_block(sites, callable_, travs))
        want += [f"{int(c)} {int(o)}" for c, o in zip(cand, off)]
    for _ in range(300):
        f = rng.randint(0, 20)
        l = f + rng.randint(1, 6)
        hosts = []
        for _ in range(rng.randint(0, 6)):
            hf = rng.randint(0, 22)
            hosts.append((hf, hf + rng.randint(1, 12), rng.randint(0, 5)))
        blocks.append("\n".join([f"hosts {f} {l} {len(hosts)}"] + ["%d %d %d" % h for h in hosts]))
        ok = [(hl - hf, q, x) for x, (hf, hl, q) in enumerate(hosts) if F.encloses(hf, hl, f, l)]
        want.append("-1 -1" if not ok else "%d %d" % min(ok)[1:])
    assert run(offref_check, blocks) == want

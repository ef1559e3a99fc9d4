"""The requests of the call-mode tests (tests/test_call_modes.py on the CPU, test_which_modes_combine of tests/test_gpu_call.py on
the GPU): every pair of modes and every (mode, profile), how `povu call` and HipDecomposer.call are asked for each, and what each
side answers.  The answers are tests/golden/call_modes.json: for all 2^7 sets of modes under each of the 5 profiles the first
refusal of the library and of the command line ("" where the request is accepted), recorded from the build that still had the
refusals written out pair by pair in check_call_inputs and parse_call_args.  No copy of the rules lives here."""
import functools
import itertools
import json
import os
import subprocess

import numpy as np

import cluster_cases as CC
import vcf_ref as V
from povu_amd import hip as H
from povu_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
GOLDEN = os.path.join(ROOT, "tests", "golden", "call_modes.json")
MODES = ("inversions", "nested", "merge", "offref", "untangle", "regions", "cluster")  # in the order of modes::Mode
PROFILES = ("raw-graph", "top-level-only", "popped", "left-normalized", "decomposed")
REGION = CC.HG1 + ":1-2"
CLI = dict(inversions=["--inversions"], nested=["--nested"], merge=["--merge-primitives"], offref=["--off-reference"], untangle=["--untangle"],
           regions=["--region", REGION], cluster=["--cluster", "0.9"])
T_FLAG = dict(inversions=H.T_INVERSIONS, nested=H.T_NESTED, merge=H.T_MERGE, offref=H.T_OFFREF, untangle=H.T_UNTANGLE)
# (modes, profile): every pair of modes without a profile, every mode under every profile
REQUESTS = [(pair, None) for pair in itertools.combinations(MODES, 2)] + [((m,), p) for m in MODES for p in PROFILES]
NO_FOREST = "cannot open the forest directory"


@functools.lru_cache(maxsize=None)
def golden():
    """{(set of modes as bits of MODES, profile number): (the library's refusal, the command line's)}"""
    g = json.load(open(GOLDEN))
    assert tuple(g["modes"]) == MODES and tuple(g["profiles"]) == PROFILES and len(g["library"]) == len(g["command_line"]) == 2 ** len(MODES) * len(PROFILES)
    return {(k % 2 ** len(MODES), k // 2 ** len(MODES)): (g["texts"][a], g["texts"][b]) for k, (a, b) in enumerate(zip(g["library"], g["command_line"]))}


def expected(modes, profile):
    return golden()[sum(1 << MODES.index(m) for m in modes), PROFILES.index(profile or "raw-graph")]


def cli_args(modes, profile):
    return [x for m in modes for x in CLI[m]] + (["--profile", profile] if profile else [])


def library_kwargs(modes, profile):
    return dict(flags=sum(T_FLAG.get(m, 0) for m in modes), profile=profile, regions=[REGION] if "regions" in modes else None,
                cluster="0.9" if "cluster" in modes else None)


def cli_answer(modes, profile):
    """What `povu call` says to the request with a forest directory that does not exist: its refusal of the modes, or "" when it
    got past its arguments (and failed on the directory, before any GPU is opened)."""
    r = subprocess.run([POVU, "call", "-i", CC.GFA, "-f", os.path.join(ROOT, "tests", "no-such-forest"), "-P", "HG1", *cli_args(modes, profile)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (modes, profile, r.stderr)
    if NO_FOREST in r.stderr:
        return ""
    assert "Flag '" in r.stderr, r.stderr
    return r.stderr[r.stderr.index("Flag '"):].strip()


def resident_example(d):
    """The worked example of the clustered calls (six segments) resident in the HipDecomposer `d`: graph, paths and sequences;
    its forest."""
    names, paths, seqs = V.read_gfa(CC.GFA)
    ids = sorted(seqs)
    at = {v: k for k, v in enumerate(ids)}
    links = [ln.split("\t") for ln in open(CC.GFA) if ln.startswith("L\t")]
    side = lambda o, plus: [plus if f == "+" else W.L + W.R - plus for f in o]  # noqa: E731
    g = W._mk(np.array(ids), np.array([at[int(f[1])] for f in links]), np.array(side([f[2] for f in links], W.R)),
              np.array([at[int(f[3])] for f in links]), np.array(side([f[4].strip() for f in links], W.L)))
    d.upload(g)
    forest = d.decompose()
    d.upload_paths(W._paths(names, [([i for i, _ in st], [r for _, r in st]) for st in paths]))
    d.upload_sequences([seqs[i] for i in g.vid.tolist()])
    return forest

"""The context's arena table (povu_hip_arena_report, HipDecomposer.arenas) and the promise of release_workspace: the table
is total and named; on one context every family of arenas fills when its call runs, and release_workspace gives every
workspace arena back and leaves the resident ones alone; every call repeated after the release returns what it returned
before; the debug exports end with the release; the wave walk's arena comes and goes with the rest."""
import numpy as np
import pytest

import class_walk_cases as K
import untangle_cases as UC
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W
from test_gpu_norm import _setup

pytestmark = pytest.mark.gpu

DATE = "00000000"
REFS = ["hap0#"]
RESIDENT = {"graph_arena", "paths_buf", "seq_buf", "shard_buf", "part_arena"}
SUB = tuple("ws_sub." + k for k in ("tables", "concealed", "smothered", "xspace", "children", "out"))


def _digest(x):
    """every array of a result as bytes, every counter, and the VCF text of a call (the device time left out)"""
    d = {k: v.tobytes() if isinstance(v, np.ndarray) else v for k, v in vars(x).items()
         if isinstance(v, (np.ndarray, int, bool, list, str)) and not k.startswith("_")}
    assert any(isinstance(v, bytes) for v in d.values())
    if isinstance(x, H.Calls):
        d["vcf"] = x.vcf_text(date=DATE)
    return d


def _call(flags=0, profile=None):
    return lambda d, f, vcf: d.call(f, REFS, flags=flags, profile=profile)


# (step, the arenas that hold bytes behind it, the call: (context, forest, VCF text of the step "call") -> result)
STEPS = (
    ("walks", ("wk_ws", "wk_out"), lambda d, f, vcf: d.walks(f)),
    ("traversals", ("tr_ws", "tr_task", "tr_trav", "tr_steps"), lambda d, f, vcf: d.traversals(f)),
    ("call", ("cl_ws", "cl_slot", "cl_rec", "cl_spell", "cl_bytes"), _call()),
    ("inversions", ("iv_ws", "iv_heads", "iv_rows"), _call(H.T_INVERSIONS)),
    ("nested", ("ns_idx", "ns_cls", "ns_ws", "ns_rec"), _call(H.T_NESTED)),
    ("left-normalized", ("nm_ws",), _call(profile="left-normalized")),
    # (pr_slab holds the codes of the pairs too long for the in-register aligner: this input has none, so the next step
    # sends every pair there)
    ("decomposed", ("pr_ws", "pr_rows"), _call(profile="decomposed")),
    ("decomposed, tier 2", ("pr_ws", "pr_slab", "pr_rows"), _call(H.T_FORCE_TIER2, "decomposed")),
    ("merge", ("mg_ws", "mg_rows"), _call(H.T_MERGE, "decomposed")),
    # (or_inv holds the inversion records' numbers among the calling paths: carved only with T_INVERSIONS, the next step)
    ("offref", ("or_ws", "or_view", "or_host", "or_rows"), _call(H.T_OFFREF)),
    ("offref, inversions", ("or_ws", "or_view", "or_inv", "or_host", "or_rows"), _call(H.T_OFFREF | H.T_INVERSIONS)),
    ("untangle", ("un_ws", "un_task", "un_part", "un_pair", "un_rows"), _call(H.T_UNTANGLE)),
    ("check_vcf", ("vc_ws", "vc_hit"), lambda d, f, vcf: d.check_vcf(vcf, spelling=True)),
)


def _bytes(report):
    return {a["name"]: a["bytes"] for a in report}


def _run_steps(d, f, snap=None):
    out, vcf = {}, None
    for name, _, run in STEPS:
        r = run(d, f, vcf)
        out[name] = _digest(r)
        if name == "call":
            vcf = out[name]["vcf"]
        if snap is not None:
            snap[name] = _bytes(d.arenas())
    return out


@pytest.fixture(scope="module")
def session():
    """One context through every family, the release, and every call again; the tests look at what it recorded."""
    d = HipDecomposer(0)
    try:
        s = dict(fresh=d.arenas(), snap={})
        d.upload(W.chain_of_bubbles(60))
        d.decompose(flags=H.F_SUBFLUBBLES)
        s["snap"]["-s"] = _bytes(d.arenas())  # (the next pass, without -s, gives ws_leaf and the six of ws_sub back itself)
        g, p = W.vntr_haplotypes(20, 8, 5, 11, reverse_every=4)
        f = _setup(d, g, UC.sequences(g, 5), p)[0]
        s["snap"]["decompose"] = _bytes(d.arenas())
        s["texts"] = f.texts()
        s["first"] = _run_steps(d, f, s["snap"])
        s["stack_before"] = d.debug_stack(0)
        s["before"] = d.arenas()
        d.release_workspace()
        s["after"] = d.arenas()
        try:
            s["stack_after"] = d.debug_stack(0)
        except RuntimeError as e:
            s["stack_after"] = str(e)
        s["again"] = _run_steps(d, f)
        s["texts_again"] = d.decompose().texts()
        yield s
    finally:
        d.close()


def test_the_table_is_total_and_named(session):
    fresh = session["fresh"]
    names = [a["name"] for a in fresh]
    assert len(fresh) == 54 and len(set(names)) == 54
    assert {a["name"] for a in fresh if a["resident"] == 1} == RESIDENT
    assert all(a["resident"] in (0, 1) for a in fresh)
    assert [a["bytes"] for a in fresh] == [0] * 54
    assert set(SUB) <= set(names) and all(x in names for _, family, _ in STEPS for x in family)


def test_every_family_shows_up(session):
    snap = session["snap"]
    assert all(snap["-s"][k] > 0 for k in SUB + ("ws_leaf", "ws", "ws2")), snap["-s"]
    assert all(snap["decompose"][k] == 0 for k in SUB + ("ws_leaf",))  # (a pass without -s keeps neither)
    assert all(snap["decompose"][k] > 0 for k in ("ws", "ws2", "graph_arena", "paths_buf", "seq_buf"))
    for name, family, _ in STEPS:
        assert all(snap[name][k] > 0 for k in family), (name, {k: snap[name][k] for k in family})


def test_then_everything_goes_back(session):
    before, after = session["before"], session["after"]
    assert [a["name"] for a in after] == [a["name"] for a in before]
    assert all(_bytes(before)[k] > 0 for _, family, _ in STEPS for k in family)  # (every family is still there to give back)
    for b, a in zip(before, after):
        assert a["bytes"] == (b["bytes"] if a["resident"] else 0), (b, a)
    assert all(_bytes(after)[k] > 0 for k in ("graph_arena", "paths_buf", "seq_buf"))


def test_nothing_dangles(session):
    assert session["first"].keys() == session["again"].keys() == {name for name, _, _ in STEPS}
    for name in session["first"]:
        assert session["again"][name] == session["first"][name], name
    assert session["texts_again"] == session["texts"] and session["texts"]


def test_debug_exports_end(session):
    assert session["stack_before"]["tree_vtx"].size > 0  # (there was state to export)
    assert session["stack_after"] == "no decompose state"


def test_the_wave_walks_arena():
    d = HipDecomposer(0)
    try:
        d.upload(K.CASES["lists_doubled"]())  # the smallest case with a class of more than 256 sides (258: a star of 128 arms)
        d.decompose()
        assert _bytes(d.arenas())["ws_walk"] > 0
        d.release_workspace()
        assert _bytes(d.arenas())["ws_walk"] == 0
    finally:
        d.close()

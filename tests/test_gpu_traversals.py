"""GPU traversals (povu_hip_forest_traversals) against the plain-Python restatement (tests/traversals_ref.py), array for
array: every graph family, random-walk / noise / reversed paths, plain and -s forests, both scan tiers, a small max_steps,
forced hash collisions, the refusals, two graphs in one context, a cross-check against the walks, and the golden GFAs
through the FFI and the CLI."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import traversals_ref as R
import walks_ref as WR
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
KEYS = ("trav_off", "allele_off", "status", "path", "first", "last", "allele", "reverse", "step_off", "step_id", "step_or")


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def _queries(f, sub):
    qs = []
    for i in range(len(f)):
        if sub:
            t = f.subtree(i)
            qs += [((int(t["id1"][v]), int(t["or1"][v])), (int(t["id2"][v]), int(t["or2"][v]))) for v in range(1, t["n_total"])]
        else:
            t = f.tree(i)
            qs += WR.queries_of_arrays(t.a_id, t.a_or, t.z_id, t.z_or)
    return qs


def _paths_of(p):
    """step lists of a workloads.Paths record (a list of step lists is returned as it is)"""
    return p if isinstance(p, list) else R.paths_from_arrays(p.off, p.ids, p.rev)


def _check(d, g, paths, flags=0, force2=False, max_steps=R.DEFAULT_MAX_STEPS):
    d.upload(g)
    f = d.decompose(flags=flags)
    d.upload_paths(paths)
    t = d.traversals(f, max_steps=max_steps, flags=H.T_FORCE_TIER2 if force2 else 0)
    qs = _queries(f, bool(flags & H.F_SUBFLUBBLES))
    assert t.n_queries == len(qs)
    want = R.flat(R.PathIndex(_paths_of(paths)), qs, max_steps)
    for k in KEYS:
        assert np.array_equal(getattr(t, k), want[k]), k
    if force2:
        assert t.n_tier2 >= t.n_traversals
    return f, t, qs


def _mixed_paths(g, seed, n_walk=6, length=60):
    """random-walk paths, noise paths and the first random walks again written reversed"""
    rw = W.random_walk_paths(g, n_walk, length, seed)
    nz = W.noise_paths(g, 3, length, seed + 1)
    steps = _paths_of(rw) + _paths_of(nz) + [[(i, 1 - o) for i, o in reversed(s)] for s in _paths_of(rw)[:2]]
    return steps


def _graphs():
    return dict(chain=W.chain_of_bubbles(300), towers=W.nested_towers(4, 3), hprc=W.hprc_shaped([300, 120], seed=3, tiny=5),
                zoo=W.bubble_zoo(6, 8, 3), tangled=W.hprc_tangled(600, seed=5, tangle_every=150, max_tangle=400),
                random=W.random_bidirected(80, 120, 5))


@pytest.mark.parametrize("force2", [False, True])
@pytest.mark.parametrize("name", ["chain", "towers", "hprc", "zoo", "tangled", "random"])
def test_graph_families_both_tiers(hip, name, force2):
    g = _graphs()[name]
    f, t, _ = _check(hip, g, _mixed_paths(g, 11), force2=force2)
    assert t.n_queries > 0 or name == "random"  # (a random bidirected graph this small may have no flubble)


def test_chain_haplotypes_with_reversed_ones(hip):
    k = 2000
    g = W.chain_of_bubbles(k)
    hp = W.chain_haplotypes(k, 12, seed=4)
    f, t, qs = _check(hip, g, hp)
    # every haplotype crosses every unit once: 12 traversals a unit, a quarter of them reverse, at most three alleles
    assert t.n_traversals == 12 * len(qs)
    assert int(t.reverse.sum()) == 3 * len(qs)
    assert np.all(np.diff(t.allele_off.astype(np.int64)) <= 3) and not t.status.any()
    a, tr, st = t.of(0, 1)
    assert len(tr) == 12 and 1 <= len(a) <= 3 and tr[0][4] == 0


def test_subflubble_forests(hip):
    for g in (W.bubble_zoo(6, 8, 3), W.bubble_zoo(8, 8, 5)):
        f, t, qs = _check(hip, g, _mixed_paths(g, 3), flags=H.F_SUBFLUBBLES)
        assert len(qs) > sum(len(f.tree(i).a_id) - 1 for i in range(len(f)))
        _check(hip, g, _mixed_paths(g, 3), flags=H.F_SUBFLUBBLES, force2=True)


def test_long_scans_go_to_tier2_and_small_max_steps(hip):
    # paths that run far between the boundaries of one flubble: tier 1 hands them over, and small max_steps cut them
    g = W.hprc_shaped([400], seed=9, tiny=5)
    hip.upload(g)
    (s, z) = _queries(hip.decompose(), False)[0]
    filler = [(int(i), int(i) % 2) for i in g.vid.tolist() if int(i) not in (s[0], z[0])]
    long_fwd = [s] + filler[:150] + [z]
    long_rev = [R.flip(z)] + filler[150:230] + [R.flip(s)]
    long_open = [s] + filler[:200]
    paths = [long_fwd, long_rev, long_open] + _paths_of(W.random_walk_paths(g, 8, 400, 21))
    f, t, _ = _check(hip, g, paths)
    assert t.n_tier2 >= 3
    al, tr, st = t.of(0, 1)
    assert (0, 0, 151, "+", 0) in tr and (1, 0, 81, "-", 1) in tr and st & H.TRAV_OPEN
    for ms in (2, 5, 70, 151, 152):
        f, t, _ = _check(hip, g, paths, max_steps=ms)
        assert (t.status & H.TRAV_LONG).any()
    _check(hip, g, paths, max_steps=70, force2=True)


def test_every_status_bit_appears(hip):
    g = W.chain_of_bubbles(200)
    f, t, _ = _check(hip, g, _paths_of(W.noise_paths(g, 10, 200, 5, jump=0.3)), max_steps=4)
    bits = int(np.bitwise_or.reduce(t.status))
    assert bits == H.TRAV_LONG | H.TRAV_STRAY | H.TRAV_OPEN


def test_hash_collisions_keep_the_exact_answer(hip, monkeypatch):
    g = W.hprc_shaped([300, 120], seed=3, tiny=5)
    paths = _paths_of(W.random_walk_paths(g, 24, 200, 8))
    hip.upload(g)
    f = hip.decompose()
    hip.upload_paths(paths)
    full = hip.traversals(f)
    assert full.n_hash_splits == 0
    monkeypatch.setenv("POVU_HIP_TRAV_HASH_BITS", "4")
    f2, t, _ = _check(hip, g, paths)
    assert t.n_hash_splits > 0
    for k in KEYS:
        assert np.array_equal(getattr(t, k), getattr(full, k)), k
    _check(hip, g, paths, force2=True)


def test_refusals(hip):
    g = W.chain_of_bubbles(50)
    hip.upload(g)
    f = hip.decompose()
    with pytest.raises(RuntimeError, match="no paths are resident"):
        hip.traversals(f)
    hip.upload_paths(W.chain_haplotypes(50, 2, 1))
    hip.traversals(f)
    with pytest.raises(RuntimeError, match="path 1 step 3: segment 999 is not in the resident graph"):
        hip.upload_paths([[(1, 0), (2, 0)], [(1, 0), (2, 0), (3, 0), (999, 0)]])
    with pytest.raises(RuntimeError, match="no paths are resident"):
        hip.traversals(f)  # (a refused upload leaves none)
    with pytest.raises(ValueError):
        hip.traversals(f, max_steps=1)
    hip.upload(g)  # the paths belong to the previous upload
    with pytest.raises(RuntimeError, match="uploaded again"):
        hip.traversals(f)
    f2 = hip.decompose()
    with pytest.raises(RuntimeError, match="no paths are resident"):
        hip.traversals(f2)
    hip.upload_paths(W.chain_haplotypes(50, 2, 1))
    fs = hip.decompose(rank=0, world=2)
    with pytest.raises(RuntimeError, match="sharded"):
        hip.traversals(fs)
    merged = hip.merge_forests([f2.pack()])
    with pytest.raises(RuntimeError, match="merged"):
        hip.traversals(merged)
    other = HipDecomposer(0)
    try:
        other.upload(g)
        other.upload_paths(W.chain_haplotypes(50, 2, 1))
        with pytest.raises(RuntimeError, match="another context"):
            other.traversals(f2)
    finally:
        other.close()
    # ids that do not ascend with the vertex index
    bad = W._mk(np.array([5, 3, 9], np.uint32), [0, 1], [W.R, W.R], [1, 2], [W.L, W.L])
    hip.upload(bad)
    with pytest.raises(RuntimeError, match="ascend"):
        hip.upload_paths([[(5, 0), (3, 0)]])


def test_two_graphs_in_one_context(hip):
    # different graphs with different paths, one after the other on one context, then the first again (stale workspace)
    g1, g2 = W.hprc_shaped([500, 200], seed=7, tiny=5), W.bubble_zoo(8, 8, 5)
    p1, p2 = _mixed_paths(g1, 31, n_walk=10, length=120), _mixed_paths(g2, 32)
    _, a, _ = _check(hip, g1, p1)
    _check(hip, g2, p2)
    _check(hip, g2, p2, flags=H.F_SUBFLUBBLES)
    _, b, _ = _check(hip, g1, p1)
    for k in KEYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("name", ["chain", "hprc", "zoo", "towers"])
def test_traversals_match_the_walks(hip, name):
    g = _graphs()[name]
    paths = _paths_of(W.random_walk_paths(g, 12, 150, 41))  # (paths that follow the links)
    hip.upload(g)
    f = hip.decompose()
    hip.upload_paths(paths)
    t = hip.traversals(f)
    w = hip.walks(f)
    checked = 0
    for q in range(t.n_queries):
        if w.status[q] & (H.WALK_MORE | H.WALK_BUDGET):
            continue
        walks = w.walks_of_query(q)
        for a in range(int(t.allele_off[q]), int(t.allele_off[q + 1])):
            b, e = int(t.step_off[a]), int(t.step_off[a + 1])
            seq = [(int(i), ">" if o == 0 else "<") for i, o in zip(t.step_id[b:e].tolist(), t.step_or[b:e].tolist())]
            if len({i for i, _ in seq}) != len(seq) or len(seq) > WR.DEFAULTS["max_steps"]:
                continue
            assert seq in walks, (q, seq)
            checked += 1
    assert checked > 0


# ---- golden GFAs with P / W lines, through the FFI and the CLI

class _Step(C.Structure):
    _fields_ = [("vertex_id", C.c_uint64), ("orientation", C.c_int)]


class _Path(C.Structure):
    _fields_ = [("name", C.c_char_p), ("name_len", C.c_size_t), ("steps", C.POINTER(_Step)), ("steps_count", C.c_size_t)]


class _Trav(C.Structure):
    _fields_ = [("path", C.c_size_t), ("first", C.c_size_t), ("last", C.c_size_t), ("reverse", C.c_int), ("allele", C.c_size_t)]


class _FlubbleTravs(C.Structure):
    _fields_ = [("traversals", C.POINTER(_Trav)), ("traversals_count", C.c_size_t), ("alleles", C.POINTER(C.POINTER(_Step))),
                ("allele_lengths", C.POINTER(C.c_size_t)), ("alleles_count", C.c_size_t), ("status", C.c_uint32)]


def _golden_gfas(golden_dir):
    out = [os.path.join(golden_dir, "gfa", "LPA.gfa")]
    out += sorted(glob.glob(os.path.join(golden_dir, "gfa", "downstream_repetitive", "*.gfa")))
    return out


def _ffi_paths(lib, gh):
    n = C.c_size_t(0)
    ps = lib.povu_graph_get_paths(gh, C.byref(n))
    names, steps = [], []
    for k in range(n.value):
        names.append(ps[k].name[:ps[k].name_len].decode() if ps[k].name else "")
        steps.append([(int(ps[k].steps[j].vertex_id), int(ps[k].steps[j].orientation)) for j in range(ps[k].steps_count)])
    lib.povu_paths_free(ps, n)
    return names, steps


def _cli_trav(gfa, out_dir, *flags):
    r = subprocess.run([POVU, "decompose", "-i", gfa, "-o", str(out_dir), "--traversals", *flags], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    comps = sorted(int(os.path.basename(p)[:-5]) for p in glob.glob(os.path.join(str(out_dir), "*.pvst")))
    assert comps and all(os.path.exists(os.path.join(str(out_dir), f"{c}.trav")) for c in comps)
    return comps


def _trav_lines(index, names, qs_text, max_steps=R.DEFAULT_MAX_STEPS):
    """the .trav text the restatement gives for one PVST text"""
    out = []
    v = 0
    for line in qs_text.splitlines():
        f = line.split("\t")
        if f[0] in ("H", "D") or len(f) < 3:
            continue
        v = int(f[1])
        (s, z), = WR.queries_of_pvst_text("F\t0\t" + f[2])
        al, tr, _ = R.traversals_of(index, s, z, max_steps)
        for k, a in enumerate(al):
            out.append(f"A\t{v}\t{f[2]}\t{k}\t{R.as_text(a)}")
        for pi, i, j, rev, a in tr:
            out.append(f"T\t{v}\t{f[2]}\t{a}\t{names[pi]}\t{i}\t{j}\t{'-' if rev else '+'}")
    return out


def test_golden_gfas_through_the_ffi_and_the_cli(golden_dir, tmp_path):
    from test_cabi_and_host import _Err, _ffi
    lib = _ffi()
    lib.povu_graph_get_paths.restype = C.POINTER(_Path)
    lib.povu_graph_get_paths.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.povu_paths_free.argtypes = [C.POINTER(_Path), C.c_size_t]
    lib.povu_flubbles_get_traversals.restype = C.POINTER(_FlubbleTravs)
    lib.povu_flubbles_get_traversals.argtypes = [C.c_void_p, C.c_size_t]
    lib.povu_flubble_traversals_free.argtypes = [C.POINTER(_FlubbleTravs)]
    lib.povu_flubbles_free.argtypes = [C.c_void_p]
    n_trav = 0
    for gfa in _golden_gfas(golden_dir):
        err = _Err(0, None)
        gh = lib.povu_graph_from_gfa(gfa.encode(), C.byref(err))
        assert gh, err.message
        names, steps = _ffi_paths(lib, gh)
        assert steps, gfa
        index = R.PathIndex(steps)
        out = tmp_path / os.path.basename(gfa)
        out.mkdir()
        comps = _cli_trav(gfa, out)
        texts = [open(out / f"{c}.pvst").read() for c in comps]
        # the CLI: one .trav per component, the restatement fed from the PVST files and the parsed paths
        for c, text in zip(comps, texts):
            got = open(out / f"{c}.trav").read().splitlines()
            assert got == _trav_lines(index, names, text), (gfa, c)
            n_trav += sum(1 for x in got if x.startswith("T"))
        # the FFI: flubble i = the PVST vertices of the trees side by side
        qs = [q for text in texts for q in WR.queries_of_pvst_text(text)]
        fl = lib.povu_graph_find_flubbles(gh, C.byref(err))
        assert fl, err.message
        assert lib.povu_flubbles_count(fl) == len(qs) + 1
        assert not lib.povu_flubbles_get_traversals(fl, 0)
        assert not lib.povu_flubbles_get_traversals(fl, len(qs) + 1)
        for i, (s, z) in enumerate(qs, start=1):
            p = lib.povu_flubbles_get_traversals(fl, i)
            assert p, (gfa, i)
            x = p.contents
            al, tr, st = R.traversals_of(index, s, z)
            got_al = [[(x.alleles[k][j].vertex_id, x.alleles[k][j].orientation) for j in range(x.allele_lengths[k])]
                      for k in range(x.alleles_count)]
            got_tr = [(x.traversals[k].path, x.traversals[k].first, x.traversals[k].last, x.traversals[k].reverse,
                       x.traversals[k].allele) for k in range(x.traversals_count)]
            assert (got_al, got_tr, x.status) == (al, tr, st), (gfa, i)
            lib.povu_flubble_traversals_free(p)
        lib.povu_flubbles_free(fl)
        lib.povu_graph_free(gh)
    assert n_trav > 0


def test_cli_traversals_with_subflubbles(golden_dir, tmp_path):
    gfa = os.path.join(golden_dir, "gfa", "LPA.gfa")
    from test_cabi_and_host import _Err, _ffi
    lib = _ffi()
    lib.povu_graph_get_paths.restype = C.POINTER(_Path)
    lib.povu_graph_get_paths.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.povu_paths_free.argtypes = [C.POINTER(_Path), C.c_size_t]
    err = _Err(0, None)
    gh = lib.povu_graph_from_gfa(gfa.encode(), C.byref(err))
    names, steps = _ffi_paths(lib, gh)
    lib.povu_graph_free(gh)
    assert len(names) == 13
    index = R.PathIndex(steps)
    comps = _cli_trav(gfa, tmp_path, "-s")
    for c in comps:
        got = open(tmp_path / f"{c}.trav").read().splitlines()
        assert got == _trav_lines(index, names, open(tmp_path / f"{c}.pvst").read()), c
    # without the flag nothing changes: no .trav file
    plain = tmp_path / "plain"
    plain.mkdir()
    r = subprocess.run([POVU, "decompose", "-i", gfa, "-o", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not glob.glob(str(plain / "*.trav"))

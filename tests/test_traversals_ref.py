"""CPU tests of the traversal restatement (tests/traversals_ref.py) on hand-traced cases, and the exported symbols of the
traversal entry points.  The GPU traversals are compared with this restatement in test_gpu_traversals.py."""
import ctypes as C
import os

import numpy as np
import pytest

import traversals_ref as R
from povu_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def p(text):
    """'>1>2<3' -> [(1, 0), (2, 0), (3, 1)]"""
    out, i = [], 0
    while i < len(text):
        o = 0 if text[i] == ">" else 1
        j = i + 1
        while j < len(text) and text[j] not in "<>":
            j += 1
        out.append((int(text[i + 1:j]), o))
        i = j
    return out


def trav(paths, s, z, max_steps=R.DEFAULT_MAX_STEPS):
    al, tr, st = R.traversals_of(R.PathIndex([p(x) for x in paths]), s, z, max_steps)
    return [R.as_text(a) for a in al], tr, st


S1, Z4 = (1, 0), (4, 0)


def test_forward_traversals_and_alleles_in_first_traversal_order():
    al, tr, st = trav([">1>3>4", ">1>2>4", ">1>3>4"], S1, Z4)
    assert al == [">1>3>4", ">1>2>4"]
    assert tr == [(0, 0, 2, 0, 0), (1, 0, 2, 0, 1), (2, 0, 2, 0, 0)]
    assert st == 0


def test_reverse_traversal_reads_s_to_z_and_shares_the_allele():
    # path 1 is path 0 written backwards: <4<2<1 starts with flip(Z) = <4 and closes on flip(S) = <1
    al, tr, st = trav([">1>2>4", "<4<2<1"], S1, Z4)
    assert al == [">1>2>4"]
    assert tr == [(0, 0, 2, 0, 0), (1, 0, 2, 1, 0)]
    assert st == 0
    # a reverse traversal alone still reads from S to Z, orientations flipped
    al, tr, _ = trav([">0<4>3<1>9"], S1, Z4)
    assert al == [">1<3>4"] and tr == [(0, 1, 3, 1, 0)]


def test_path_that_passes_s_twice():
    # >1 >2 >1 >3 >4: the scan from position 0 meets segment 1 again (>1 is not Z): STRAY; the one from 2 closes
    al, tr, st = trav([">1>2>1>3>4"], S1, Z4)
    assert al == [">1>3>4"] and tr == [(0, 2, 4, 0, 0)]
    assert st == R.STRAY


def test_nested_flubbles_sharing_a_boundary():
    # outer (1, 6) holds (1, 4) and (4, 6); a path through all of them
    path = [">1>2>4>5>6"]
    assert trav(path, S1, (6, 0))[:2] == ([">1>2>4>5>6"], [(0, 0, 4, 0, 0)])
    assert trav(path, S1, Z4)[:2] == ([">1>2>4"], [(0, 0, 2, 0, 0)])
    assert trav(path, (4, 0), (6, 0))[:2] == ([">4>5>6"], [(0, 2, 4, 0, 0)])


def test_stray_long_open():
    # STRAY: S's segment the other way round (flip(S) starts nothing)
    assert trav([">1>2<1>3"], S1, Z4) == ([], [], R.STRAY)
    # Z's segment the other way round is a stray end of the forward scan, and flip(Z) starts a reverse scan that runs off
    assert trav([">1>2<4"], S1, Z4) == ([], [], R.STRAY | R.OPEN)
    # OPEN: the path ends before either boundary segment comes back
    assert trav([">1>2>3"], S1, Z4) == ([], [], R.OPEN)
    # LONG: with max_steps 3 the scan would need four steps, and the path goes on at position 3
    assert trav([">1>2>3>4"], S1, Z4, max_steps=3) == ([], [], R.LONG)
    assert trav([">1>2>3>4"], S1, Z4, max_steps=4)[1] == [(0, 0, 3, 0, 0)]
    # the path ending exactly at the window's end is OPEN, not LONG
    assert trav([">1>2>3"], S1, Z4, max_steps=3) == ([], [], R.OPEN)
    # reverse scans set the bits too: <4 then <1 the wrong way round
    assert trav(["<4>2>1"], S1, Z4) == ([], [], R.STRAY | R.OPEN)  # (and >1 starts a forward scan that runs off the end)


def test_same_segment_boundaries_have_no_traversal():
    assert trav([">1>2>1"], S1, (1, 1)) == ([], [], 0)


def test_flat_arrays_layout():
    idx = R.PathIndex([p(">1>2>4>5>6"), p("<6<5<4<3<1")])
    f = R.flat(idx, [(S1, Z4), ((4, 0), (6, 0)), (S1, (1, 0))])
    assert f["trav_off"].tolist() == [0, 2, 4, 4]
    assert f["allele_off"].tolist() == [0, 2, 3, 3]
    assert f["path"].tolist() == [0, 1, 0, 1] and f["reverse"].tolist() == [0, 1, 0, 1]
    assert f["first"].tolist() == [0, 2, 2, 0] and f["last"].tolist() == [2, 4, 4, 2]
    assert f["allele"].tolist() == [0, 1, 0, 0]
    assert f["step_off"].tolist() == [0, 3, 6, 9]
    assert R.as_text(zip(f["step_id"][3:6].tolist(), f["step_or"][3:6].tolist())) == ">1>3>4"


def test_chain_haplotypes_follow_the_links():
    g = W.chain_of_bubbles(50)
    hp = W.chain_haplotypes(50, 8, seed=3)
    succ = {}
    for a, sa, b, sb in zip(g.v1.tolist(), g.s1.tolist(), g.v2.tolist(), g.s2.tolist()):
        succ.setdefault((int(g.vid[a]), sa), set()).add((int(g.vid[b]), 0 if sb == W.L else 1))
        succ.setdefault((int(g.vid[b]), sb), set()).add((int(g.vid[a]), 0 if sa == W.L else 1))
    for k in range(len(hp)):
        s = hp.steps(k)
        for x, y in zip(s, s[1:]):  # leaving x by its exit side (r for '>') reaches y
            assert y in succ[(x[0], W.R if x[1] == 0 else W.L)]
    # every unit of every haplotype is one traversal of the unit's flubble
    idx = R.PathIndex([hp.steps(k) for k in range(len(hp))])
    al, tr, st = R.traversals_of(idx, (1, 0), (4, 0))
    assert len(tr) == 8 and st == 0 and 1 <= len(al) <= 3


def test_paths_gfa_lines():
    hp = W.Paths(["a", "b"], np.array([0, 2, 3], np.uint64), np.array([1, 2, 3], np.uint32), np.array([0, 1, 0], np.uint8))
    assert hp.to_gfa() == "P\ta\t1+,2-\t*\nP\tb\t3+\t*\n"


def test_libraries_export_the_traversal_entry_points():
    hip = C.CDLL(os.path.join(ROOT, "povu_amd", "lib", "libpovu_hip.so"))
    ffi = C.CDLL(os.path.join(ROOT, "povu_amd", "lib", "libpovu_ffi.so"))
    for name in ("povu_hip_paths_upload", "povu_hip_forest_traversals", "povu_hip_traversals_free"):
        assert hasattr(hip, name), name
    for name in ("povu_flubbles_get_traversals", "povu_flubble_traversals_free"):
        assert hasattr(ffi, name), name

"""CPU tests of the drop-in boundary: the C-ABI libraries load and export every declared symbol, the
host-side pieces (GFA tokenizer, FFI graph builder, PVST serialiser, CLI argument handling) behave
like the reference, and compute entry points fail loudly without a GPU."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from povu_amd import hip as H
from povu_amd import workloads as W
from test_oracle import _load_gfa_links, dump_component

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "povu_amd", "lib")
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")


def _built():
    if not (os.path.exists(os.path.join(LIB, "libpovu_hip.so")) and os.path.exists(os.path.join(LIB, "libpovu_ffi.so"))
            and os.path.exists(POVU)):
        import __graft_entry__
        __graft_entry__.build()


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(povu_[a-z0-9_]+)\s*\(", txt)))


def test_hip_library_exports_every_declared_symbol():
    _built()
    lib = C.CDLL(os.path.join(LIB, "libpovu_hip.so"))
    names = _declared("povu_hip.h")
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), n


def test_ffi_library_exports_the_reference_abi():
    _built()
    lib = C.CDLL(os.path.join(LIB, "libpovu_ffi.so"))
    names = _declared("povu_ffi.h")
    reference_33 = """povu_graph_new povu_graph_from_gfa povu_graph_free povu_graph_add_vertex povu_graph_add_edge
        povu_graph_add_path povu_graph_finalize povu_graph_vertex_count povu_graph_edge_count povu_graph_path_count
        povu_graph_get_vertices povu_graph_get_edges povu_graph_get_paths povu_vertices_free povu_edges_free
        povu_paths_free povu_graph_set_references_from_file povu_graph_set_references_from_prefixes
        povu_graph_find_flubbles povu_flubbles_free povu_flubbles_count povu_flubbles_get povu_flubble_free
        povu_flubbles_get_pvst_tree povu_pvst_tree_free povu_pvst_tree_vertex_count povu_flubbles_call_variants
        povu_vcf_write_to_file povu_vcf_to_string povu_vcf_free povu_string_free povu_gfa_to_vcf
        povu_error_free""".split()
    assert len(reference_33) == 33
    for n in reference_33:
        assert n in names, n
    for n in names:
        assert hasattr(lib, n), n


class _Err(C.Structure):
    _fields_ = [("code", C.c_int), ("message", C.c_char_p)]


class _Edge(C.Structure):
    _fields_ = [("from_id", C.c_uint64), ("from_o", C.c_int), ("to_id", C.c_uint64), ("to_o", C.c_int)]


class _Vertex(C.Structure):
    _fields_ = [("id", C.c_uint64), ("sequence", C.c_char_p), ("sequence_len", C.c_size_t)]


def _ffi():
    _built()
    lib = C.CDLL(os.path.join(LIB, "libpovu_ffi.so"))
    lib.povu_graph_new.restype = C.c_void_p
    lib.povu_graph_new.argtypes = [C.c_size_t] * 3
    lib.povu_graph_from_gfa.restype = C.c_void_p
    lib.povu_graph_from_gfa.argtypes = [C.c_char_p, C.POINTER(_Err)]
    lib.povu_graph_free.argtypes = [C.c_void_p]
    lib.povu_graph_add_vertex.restype = C.c_size_t
    lib.povu_graph_add_vertex.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p]
    lib.povu_graph_add_edge.restype = C.c_size_t
    lib.povu_graph_add_edge.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_int]
    lib.povu_graph_add_path.restype = C.c_bool
    lib.povu_graph_add_path.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
    for f in ("vertex", "edge", "path"):
        getattr(lib, f"povu_graph_{f}_count").restype = C.c_size_t
        getattr(lib, f"povu_graph_{f}_count").argtypes = [C.c_void_p]
    lib.povu_graph_get_edges.restype = C.POINTER(_Edge)
    lib.povu_graph_get_edges.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.povu_graph_get_vertices.restype = C.POINTER(_Vertex)
    lib.povu_graph_get_vertices.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.povu_edges_free.argtypes = [C.c_void_p, C.c_size_t]
    lib.povu_vertices_free.argtypes = [C.c_void_p, C.c_size_t]
    lib.povu_graph_find_flubbles.restype = C.c_void_p
    lib.povu_graph_find_flubbles.argtypes = [C.c_void_p, C.POINTER(_Err)]
    lib.povu_flubbles_get.restype = C.c_void_p
    lib.povu_flubbles_get.argtypes = [C.c_void_p, C.c_size_t]
    lib.povu_flubbles_count.restype = C.c_size_t
    lib.povu_flubbles_count.argtypes = [C.c_void_p]
    lib.povu_gfa_to_vcf.restype = C.c_bool
    lib.povu_gfa_to_vcf.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(_Err)]
    lib.povu_error_free.argtypes = [C.POINTER(_Err)]
    return lib


def test_ffi_builder_matches_reference_semantics():
    """povu-rs/tests/builder_tests.rs: counts, orientation mapping (FORWARD=l, REVERSE=r), stubs."""
    lib = _ffi()
    g = lib.povu_graph_new(4, 4, 0)
    for i, s in [(1, b"A"), (2, b"C"), (3, b"G"), (4, b"T")]:
        assert lib.povu_graph_add_vertex(g, i, s) == i - 1
    assert lib.povu_graph_add_vertex(g, 9, None) == C.c_size_t(-1).value
    assert lib.povu_graph_add_edge(g, 1, 0, 2, 0) == 0
    assert lib.povu_graph_add_edge(g, 1, 1, 3, 0) == 1
    assert lib.povu_graph_add_edge(g, 2, 1, 2, 1) == 2  # self loop accepted (builder_tests.rs:243-254)
    assert lib.povu_graph_add_edge(g, 1, 0, 77, 0) == C.c_size_t(-1).value  # unknown vertex id
    assert lib.povu_graph_vertex_count(g) == 4 and lib.povu_graph_edge_count(g) == 3
    assert lib.povu_graph_path_count(g) == 0
    assert lib.povu_graph_add_path(g, b"p", None, 0) is False
    n = C.c_size_t(0)
    e = lib.povu_graph_get_edges(g, C.byref(n))
    assert n.value == 3
    assert (e[1].from_id, e[1].from_o, e[1].to_id, e[1].to_o) == (1, 1, 3, 0)
    lib.povu_edges_free(e, n)
    err = _Err(0, None)
    assert lib.povu_gfa_to_vcf(b"a", b"b", None, C.byref(err)) is False and err.code == 1
    assert b"not yet implemented" in err.message
    lib.povu_graph_free(g)
    assert lib.povu_graph_vertex_count(None) == 0


def test_ffi_gfa_loader_contract(golden_dir):
    """Row A host part: vertices ascending by id, links in L order, `+`/`-` -> sides."""
    lib = _ffi()
    for path in sorted(glob.glob(os.path.join(golden_dir, "gfa", "*.gfa"))):
        name = os.path.basename(path)
        if name in ("malformed_path_missing_overlaps.gfa",):
            continue
        err = _Err(0, None)
        g = lib.povu_graph_from_gfa(path.encode(), C.byref(err))
        assert g, (name, err.message)
        want = _load_gfa_links(path)
        nv = C.c_size_t(0)
        v = lib.povu_graph_get_vertices(g, C.byref(nv))
        assert [v[i].id for i in range(nv.value)] == want.vid.tolist()
        lib.povu_vertices_free(v, nv)
        ne = C.c_size_t(0)
        e = lib.povu_graph_get_edges(g, C.byref(ne))
        got = [(e[i].from_id, e[i].from_o, e[i].to_id, e[i].to_o) for i in range(ne.value)]
        exp = [(int(want.vid[a]), int(sa), int(want.vid[b]), int(sb))
               for a, sa, b, sb in zip(want.v1, want.s1, want.v2, want.s2)]
        assert got == exp, name
        lib.povu_edges_free(e, ne)
        lib.povu_graph_free(g)


def test_ffi_gfa_errors(tmp_path):
    lib = _ffi()
    err = _Err(0, None)
    assert not lib.povu_graph_from_gfa(b"", C.byref(err)) and err.message == b"GFA path must not be empty"
    err = _Err(0, None)
    assert not lib.povu_graph_from_gfa(b"/nonexistent.gfa", C.byref(err))
    assert err.message.startswith(b"GFA file does not exist: /nonexistent.gfa")
    bad = tmp_path / "bad.gfa"
    bad.write_text("H\tVN:Z:1.0\nS\t1\t\nS\t2\tA\n")
    err = _Err(0, None)
    assert not lib.povu_graph_from_gfa(str(bad).encode(), C.byref(err))
    assert err.message == f"Invalid GFA '{bad}': S record on line 2 has an empty sequence".encode()
    # a link to a segment the file does not define: consecutive ids (plain arithmetic), dense ids (table), sparse ids (search)
    for ids, ghost in (((5, 6, 7), 4), ((5, 6, 7), 8), ((5, 6, 7), 4000000000), ((5, 7, 9), 6), ((5, 7, 900000), 8)):
        body = "".join(f"S\t{i}\tA\n" for i in ids) + f"L\t{ids[0]}\t+\t{ids[1]}\t+\t0M\nL\t{ids[1]}\t+\t{ghost}\t-\t0M\n"
        bad.write_text(body)
        err = _Err(0, None)
        assert not lib.povu_graph_from_gfa(str(bad).encode(), C.byref(err))
        assert err.message == f"Invalid GFA '{bad}': L record 1 references unknown segment {ghost}".encode(), err.message
    bad.write_text("S\t1\tA\nX\tfoo\n")
    err = _Err(0, None)
    assert not lib.povu_graph_from_gfa(str(bad).encode(), C.byref(err))
    assert err.message == f"Invalid GFA '{bad}': unsupported record type 'X' on line 2".encode()


def test_gfa_loader_with_several_tokenizer_threads(tmp_path):
    """A file large enough for several tokenizer slices (>= 4 MiB each): same graph as the generator's, and the
    first malformed record in FILE order is the one reported, with its global line number."""
    lib = _ffi()
    g = W.chain_of_bubbles(60000)  # ~10 MB of GFA text
    path = tmp_path / "big.gfa"
    text = g.to_gfa()
    path.write_text(text)
    assert len(text) > 3 * (4 << 20) // 2
    err = _Err(0, None)
    h = lib.povu_graph_from_gfa(str(path).encode(), C.byref(err))
    assert h, err.message
    assert lib.povu_graph_vertex_count(h) == g.n_vtx and lib.povu_graph_edge_count(h) == g.n_links
    ne = C.c_size_t(0)
    e = lib.povu_graph_get_edges(h, C.byref(ne))
    step = 997
    got = [(e[i].from_id, e[i].from_o, e[i].to_id, e[i].to_o) for i in range(0, ne.value, step)]
    exp = [(int(g.vid[g.v1[i]]), int(g.s1[i]), int(g.vid[g.v2[i]]), int(g.s2[i])) for i in range(0, g.n_links, step)]
    assert got == exp
    lib.povu_edges_free(e, ne)
    lib.povu_graph_free(h)
    lines = text.split("\n")
    for bad_line in (len(lines) // 5, len(lines) - 10):  # in the first slice / in the last one
        broken = list(lines)
        broken[bad_line - 1] = "L\t1\t+\t2"
        broken[len(lines) - 5] = "Q\tlater error that must not win"
        path.write_text("\n".join(broken))
        err = _Err(0, None)
        assert not lib.povu_graph_from_gfa(str(path).encode(), C.byref(err))
        assert err.message == f"Invalid GFA '{path}': malformed L record on line {bad_line}".encode(), err.message


def test_gfa_loader_line_shapes_across_slices(tmp_path):
    """The counting pass and the tokenizing pass must agree on what a record is, wherever the slices are cut: CRLF line ends,
    blank lines, L records ahead of their S records, descending ids, a header in the middle, no line feed at the end."""
    lib = _ffi()
    rng = np.random.default_rng(11)
    n = 250000
    ids = rng.permutation(np.arange(1, 3 * n, 3))[:n]  # sparse, unordered
    rows = []
    links = []
    for k in range(n):
        if k and k % 3 == 0:  # a link between two segments, possibly ahead of both S lines
            a, b = int(ids[rng.integers(0, n)]), int(ids[rng.integers(0, n)])
            sa, sb = "+-"[int(rng.integers(0, 2))], "+-"[int(rng.integers(0, 2))]
            rows.append(f"L\t{a}\t{sa}\t{b}\t{sb}\t0M" + ("\r" if k % 7 == 0 else ""))
            links.append((a, 1 if sa == "+" else 0, b, 0 if sb == "+" else 1))
        if k % 1000 == 0:
            rows.append("")  # blank line
        if k % 5000 == 1:
            rows.append("H\tVN:Z:1.0")
        rows.append(f"S\t{int(ids[k])}\t{'ACGT' * int(rng.integers(1, 20))}" + ("\tLN:i:4" if k % 13 == 0 else "") + ("\r" if k % 11 == 0 else ""))
    text = "\n".join(rows)  # (no line feed behind the last record)
    assert len(text) > 3 * (4 << 20)
    path = tmp_path / "shapes.gfa"
    path.write_bytes(text.encode())
    err = _Err(0, None)
    h = lib.povu_graph_from_gfa(str(path).encode(), C.byref(err))
    assert h, err.message
    nv = C.c_size_t(0)
    v = lib.povu_graph_get_vertices(h, C.byref(nv))
    assert [v[i].id for i in range(nv.value)] == sorted(int(x) for x in ids)
    lib.povu_vertices_free(v, nv)
    ne = C.c_size_t(0)
    e = lib.povu_graph_get_edges(h, C.byref(ne))
    assert ne.value == len(links)
    assert [(e[i].from_id, e[i].from_o, e[i].to_id, e[i].to_o) for i in range(ne.value)] == links
    lib.povu_edges_free(e, ne)
    lib.povu_graph_free(h)


def test_compute_entry_points_fail_loudly_without_gpu():
    lib = _ffi()
    hl = H.load_lib()
    if hl.povu_hip_device_count() > 0:
        pytest.skip("a GPU is visible")
    g = lib.povu_graph_new(3, 2, 0)
    for i in (1, 2, 3):
        lib.povu_graph_add_vertex(g, i, b"A")
    lib.povu_graph_add_edge(g, 1, 1, 2, 0)
    lib.povu_graph_add_edge(g, 2, 1, 3, 0)
    err = _Err(0, None)
    assert not lib.povu_graph_find_flubbles(g, C.byref(err))
    assert err.code == 1 and b"no CPU fallback" in err.message
    lib.povu_graph_free(g)
    with pytest.raises(H.HipUnavailable):
        H.HipDecomposer(0)


def test_pvst_serialiser_matches_to_pvst(golden_dir):
    """povu_hip_pvst_format (host only) on the oracle's PVST arrays == the oracle's text."""
    hl = H.load_lib()
    hl.povu_hip_pvst_format.restype = C.c_void_p
    hl.povu_hip_pvst_format.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_size_t)]
    graphs = [W.chain_of_bubbles(30), W.nested_towers(7, 2), _load_gfa_links(os.path.join(golden_dir, "gfa", "LPA.gfa")),
              _load_gfa_links(os.path.join(golden_dir, "gfa", "linear_no_variant.gfa"))]
    import test_oracle as T
    for g in graphs:
        want = O.decompose(g)[1]
        lib = O.lib()
        d = lib.orc_dump_component
        dd = T.dump_component(g, 0)
        n = len(dd["p_parent"])
        a, z, p = dd["p_a_id"].astype(np.uint32), dd["p_z_id"].astype(np.uint32), dd["p_parent"].astype(np.uint32)
        # orientations are not in the python dump dict: recover them from the expected text
        rows = want.splitlines()[1:]
        ao = np.array([0] + [1 if r.split("\t")[2][0] == "<" else 0 for r in rows[1:]], dtype=np.uint8)
        zo = np.array([0] + [1 if re.match(r"^[<>]\d+<", r.split("\t")[2]) else 0 for r in rows[1:]], dtype=np.uint8)
        ln = C.c_size_t(0)
        ptr = hl.povu_hip_pvst_format(n, a.ctypes.data, z.ctypes.data, ao.ctypes.data, zo.ctypes.data, p.ctypes.data,
                                      C.byref(ln))
        assert ptr
        got = C.string_at(ptr, ln.value).decode()
        hl.povu_hip_buffer_free(ptr)
        assert got == want


def test_pvst_serialiser_number_widths_and_fanout():
    """Every decimal width of a u32 id (1 .. 10 digits), a vertex with many children, a wide tree and a path: the text the
    serialiser writes into its one buffer against the same lines formatted here (to_pvst.cpp:23-109)."""
    hl = H.load_lib()
    hl.povu_hip_pvst_format.restype = C.c_void_p
    hl.povu_hip_pvst_format.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_size_t)]
    rng = np.random.default_rng(5)
    edge_ids = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999,
                100000000, 999999999, 1000000000, 4294967294]
    for n, shape in ((1, "path"), (2, "path"), (len(edge_ids) + 1, "star"), (1200, "path"), (5000, "random"), (100001, "star")):
        parent = np.zeros(n, dtype=np.uint32)
        for v in range(1, n):
            parent[v] = 0 if shape == "star" else v - 1 if shape == "path" else int(rng.integers(0, v))
        a = rng.integers(0, 2 ** 32 - 1, n, dtype=np.uint64).astype(np.uint32)
        z = rng.integers(0, 2 ** 32 - 1, n, dtype=np.uint64).astype(np.uint32)
        if n > len(edge_ids):
            a[1:len(edge_ids) + 1] = np.array(edge_ids, dtype=np.uint32)
            z[1:len(edge_ids) + 1] = np.array(edge_ids[::-1], dtype=np.uint32)
        ao, zo = rng.integers(0, 2, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8)
        kids = [[] for _ in range(n)]
        for v in range(1, n):
            kids[parent[v]].append(v)
        want = ["H\t0.0.3\t.\t.\t."]
        for v in range(n):
            ch = ", ".join(map(str, kids[v])) if kids[v] else "."
            if v == 0:
                want.append(f"D\t0\t.\t{ch}\t.")
            else:
                want.append(f"F\t{v}\t{'<' if ao[v] else '>'}{a[v]}{'<' if zo[v] else '>'}{z[v]}\t{ch}\tL")
        ln = C.c_size_t(0)
        ptr = hl.povu_hip_pvst_format(n, a.ctypes.data, z.ctypes.data, ao.ctypes.data, zo.ctypes.data, parent.ctypes.data, C.byref(ln))
        assert ptr
        got = C.string_at(ptr, ln.value).decode()
        hl.povu_hip_buffer_free(ptr)
        assert got == "\n".join(want) + "\n"
    # a parent that does not precede its child is refused
    bad = np.array([0, 2, 1], dtype=np.uint32)
    z3, o3 = np.zeros(3, dtype=np.uint32), np.zeros(3, dtype=np.uint8)
    assert not hl.povu_hip_pvst_format(3, z3.ctypes.data, z3.ctypes.data, o3.ctypes.data, o3.ctypes.data, bad.ctypes.data, None)


def test_cli_surface(tmp_path, golden_dir):
    _built()
    r = subprocess.run([POVU, "--version"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "0.0.1-alpha"  # app/cli/cli.hpp:10
    r = subprocess.run([POVU, "decompose"], capture_output=True, text=True)
    assert r.returncode == 1 and "required" in r.stderr
    r = subprocess.run([POVU, "call", "-i", "x"], capture_output=True, text=True)
    assert r.returncode == 1
    bad = tmp_path / "bad.gfa"
    bad.write_text("S\t1\n")
    r = subprocess.run([POVU, "decompose", "-i", str(bad), "-o", str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and f"Invalid GFA '{bad}': S record on line 1 is missing a sequence" in r.stderr
    if H.load_lib().povu_hip_device_count() == 0:
        r = subprocess.run([POVU, "decompose", "-i", os.path.join(golden_dir, "gfa", "LPA.gfa"), "-o", str(tmp_path)],
                           capture_output=True, text=True)
        assert r.returncode != 0 and "no CPU fallback" in r.stderr
        assert not list(tmp_path.glob("*.pvst"))


def test_workspace_estimate_of_the_headline_graph():
    """What one plain decompose reserves beside the resident graph, for BASELINE config 4 at full size: under 50 GB (round 3:
    80 GB) -- the parts add up, and the general case (renumbered vertices, hub vertices, self loops) costs rows A/B four
    times as much.  Host arithmetic only: no GPU."""
    lib = C.CDLL(os.path.join(LIB, "libpovu_hip.so"))
    lib.povu_hip_workspace_estimate.restype = C.c_uint64
    lib.povu_hip_workspace_estimate.argtypes = [C.c_uint32] * 3
    lib.povu_hip_workspace_breakdown.argtypes = [C.c_uint32] * 3 + [C.POINTER(C.c_uint64)]
    V, E, Cn = 99860187, 122435438, 2024
    total = lib.povu_hip_workspace_estimate(V, E, Cn)
    assert 30e9 < total < 50e9
    o = (C.c_uint64 * 7)()
    assert lib.povu_hip_workspace_breakdown(V, E, Cn, o) == 0
    assert o[0] + o[1] + o[2] + o[4] + max(o[3], o[5]) == total
    assert o[6] > 3 * o[0]
    assert lib.povu_hip_workspace_estimate(V, E, 0) > total  # (component count unknown: every segment its own)
    small = lib.povu_hip_workspace_estimate(1000, 1500, 1)
    assert 0 < small < 64 << 20


def test_workspace_sizes_match_the_recorded_bytes(golden_dir):
    """Every arena layout is a list of spans that is measured and carved by the same code, and rewriting a list must not
    move a public size: the three size functions give, to the byte, what the build of the commit named in the golden file
    gave.  The shapes are the smallest at which a max() inside the lists changes sides, plus the headline graph.  Host
    arithmetic only: no GPU."""
    import json
    _built()
    lib = C.CDLL(os.path.join(LIB, "libpovu_hip.so"))
    lib.povu_hip_workspace_estimate.restype = C.c_uint64
    lib.povu_hip_workspace_estimate.argtypes = [C.c_uint32] * 3
    lib.povu_hip_workspace_breakdown.argtypes = [C.c_uint32] * 3 + [C.POINTER(C.c_uint64)]
    lib.povu_hip_leaf_workspace_estimate.restype = C.c_uint64
    lib.povu_hip_leaf_workspace_estimate.argtypes = [C.c_uint32] * 2
    shapes = json.load(open(os.path.join(golden_dir, "workspace_bytes.json")))["shapes"]
    assert [(r["V"], r["E"], r["C"]) for r in shapes] == [
        (1, 0, 1), (3, 2, 1), (1000, 1500, 1), (1000, 1500, 0), (1000, 400, 37), (1000, 5000, 1), (70000, 90000, 70000),
        (99860187, 122435438, 2024), (99860187, 122435438, 0)]
    for r in shapes:
        V, E, Cn = r["V"], r["E"], r["C"]
        o = (C.c_uint64 * 7)()
        assert lib.povu_hip_workspace_breakdown(V, E, Cn, o) == 0
        assert list(o) == r["breakdown"], (V, E, Cn)
        assert lib.povu_hip_workspace_estimate(V, E, Cn) == r["estimate"], (V, E, Cn)
        assert lib.povu_hip_leaf_workspace_estimate(V, Cn) == r["leaf_estimate"], (V, E, Cn)


def test_cli_gpus_flag_arguments(tmp_path, golden_dir):
    """`--gpus N` (additive; default 1): which device every worker gets is settled on the host before anything touches a
    GPU -- 0 .. N-1 or the N entries of POVU_HIP_DEVICES, each checked against the visible devices -- and a multi-GPU run
    without GPUs fails as loudly as the single-GPU one."""
    _built()
    gfa = os.path.join(golden_dir, "gfa", "LPA.gfa")
    run = lambda args, **env: subprocess.run([POVU] + args, capture_output=True, text=True, env=dict(os.environ, **env))  # noqa: E731
    r = run(["decompose", "--gpus", "0", "-i", gfa])
    assert r.returncode == 1 and "between 1 and 64" in r.stderr
    r = run(["decompose", "--gpus=65", "-i", gfa])
    assert r.returncode == 1 and "between 1 and 64" in r.stderr
    r = run(["decompose", "--gpus"])
    assert r.returncode == 1 and "requires an argument" in r.stderr
    r = run(["decompose", "--gpus", "2", "-i", gfa, "-o", str(tmp_path)], POVU_HIP_DEVICES="0,0,0")
    assert r.returncode == 1 and "names 3 devices but --gpus is 2" in r.stderr
    r = run(["decompose", "--gpus", "2", "-i", gfa, "-o", str(tmp_path)], POVU_HIP_DEVICES="0;1")
    assert r.returncode == 1 and "comma-separated" in r.stderr
    n = H.load_lib().povu_hip_device_count()
    r = run(["decompose", "--gpus", str(max(n, 1) + 1), "-i", gfa, "-o", str(tmp_path)])
    assert r.returncode == 1 and f"device {n} is not visible ({n} HIP devices)" in r.stderr
    assert not list(tmp_path.glob("*.pvst"))
    r = run(["info", "--gpus", "2", "-i", gfa])  # only `decompose` takes the flag
    assert r.returncode == 1 and "could not be matched" in r.stderr


class _Doc(C.Structure):
    _fields_ = [("n", C.c_uint32), ("type", C.POINTER(C.c_char)), ("file_id", C.POINTER(C.c_uint32)),
                ("a_id", C.POINTER(C.c_uint32)), ("z_id", C.POINTER(C.c_uint32)), ("a_or", C.POINTER(C.c_uint8)),
                ("z_or", C.POINTER(C.c_uint8)), ("route", C.POINTER(C.c_uint8)), ("parent", C.POINTER(C.c_uint32)),
                ("height", C.POINTER(C.c_uint32))]


def test_pvst_write_read_round_trip(golden_dir):
    """the reader (read_pvst + comp_heights) on the writer's output."""
    hl = H.load_lib()
    hl.povu_pvst_parse.restype = C.POINTER(_Doc)
    hl.povu_pvst_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    hl.povu_pvst_doc_free.argtypes = [C.POINTER(_Doc)]
    import test_oracle as T
    for g in [W.nested_towers(9, 2), W.chain_of_bubbles(25), _load_gfa_links(os.path.join(golden_dir, "gfa", "LPA.gfa"))]:
        text = O.decompose(g)[1].encode()
        dd = T.dump_component(g, 0)
        err = C.create_string_buffer(256)
        d = hl.povu_pvst_parse(text, len(text), err, 256)
        assert d, err.value
        doc = d.contents
        n = doc.n
        assert n == len(dd["p_parent"])
        assert [doc.type[i] for i in range(n)] == [b"D"] + [b"F"] * (n - 1)
        assert [doc.file_id[i] for i in range(n)] == list(range(n))
        assert [doc.parent[i] for i in range(n)] == dd["p_parent"].tolist()
        assert [doc.a_id[i] for i in range(1, n)] == dd["p_a_id"].tolist()[1:]
        assert [doc.z_id[i] for i in range(1, n)] == dd["p_z_id"].tolist()[1:]
        assert [doc.a_or[i] for i in range(1, n)] == dd["p_a_or"].tolist()[1:]
        assert [doc.z_or[i] for i in range(1, n)] == dd["p_z_or"].tolist()[1:]
        h = [0] * n
        for i in range(1, n):
            h[i] = h[dd["p_parent"][i]] + 1
        assert [doc.height[i] for i in range(n)] == h
        hl.povu_pvst_doc_free(d)
    err = C.create_string_buffer(256)
    assert not hl.povu_pvst_parse(b"H\t0.0.2\t.\t.\t.\n", 16, err, 256) and b"Unsupported PVST version" in err.value
    assert not hl.povu_pvst_parse(b"H\t0.0.3\t.\t.\n", 12, err, 256) and b"invalid number of columns" in err.value


def test_pvst_reader_subflubble_lines():
    """A PVST as `decompose -s` writes it (src/mto/to_pvst.cpp:50-105): every vertex family of the wire format --
    D dummy, F flubble, T tiny, O parallel ("overlap"), C concealed, M midi, S smothered -- with both routes, file
    ids that are not the line order, a vertex listed before its parent and `, `-separated children.  Expected values
    follow read_pvst (src/mto/from_pvst.cpp:136-158 label and route, :284-297 children by FILE id) and comp_heights
    (include/povu/graph/pvst.hpp:807-836)."""
    hl = H.load_lib()
    hl.povu_pvst_parse.restype = C.POINTER(_Doc)
    hl.povu_pvst_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    hl.povu_pvst_doc_free.argtypes = [C.POINTER(_Doc)]
    text = ("H\t0.0.3\t.\t.\t.\n"
            "D\t0\t.\t1, 9\t.\n"
            "F\t1\t>1>40\t2, 3, 5\tL\n"
            "T\t2\t>2>4\t.\tL\n"
            "O\t3\t>5<7\t.\tR\n"
            "S\t8\t<12>13\t.\tR\n"          # listed before its parent (file id 6)
            "C\t5\t>10>20\t6,7\tL\n"        # children without the blank after the comma
            "S\t6\t>11>14\t8\tL\n"
            "M\t7\t<15<18\t.\tR\n"
            "F\t9\t<4294967294>50\t.\tL\n").encode()
    err = C.create_string_buffer(256)
    d = hl.povu_pvst_parse(text, len(text), err, 256)
    assert d, err.value
    doc = d.contents
    n = doc.n
    assert n == 9
    col = lambda name: [getattr(doc, name)[i] for i in range(n)]  # noqa: E731
    assert b"".join(col("type")) == b"DFTOSCSMF"
    assert col("file_id") == [0, 1, 2, 3, 8, 5, 6, 7, 9]
    NIL = 0xFFFFFFFF
    #            D    F1  T2  O3  S8  C5  S6  M7  F9        (vertex idx = line order)
    assert col("parent") == [NIL, 0, 1, 1, 6, 1, 5, 5, 0]
    assert col("height") == [0, 1, 2, 2, 4, 2, 3, 3, 1]
    assert col("a_id")[1:] == [1, 2, 5, 12, 10, 11, 15, 4294967294]
    assert col("z_id")[1:] == [40, 4, 7, 13, 20, 14, 18, 50]
    assert col("a_or")[1:] == [0, 0, 0, 1, 0, 0, 1, 1]
    assert col("z_or")[1:] == [0, 0, 1, 0, 0, 0, 1, 0]
    assert col("route")[1:] == [0, 0, 1, 1, 0, 0, 1, 0]
    hl.povu_pvst_doc_free(d)
    # what `decompose -s` really writes where find_concealed nests "in relation to z" (concealed.cpp:1077 hangs the concealed
    # vertex below the child flubble): vertex 3 listed under 1 AND 2, vertex 2 under nobody.  add_edge makes the last lister
    # the parent; comp_heights walks the children vectors from the root: 0 -> 1 -> 3, and never reaches 2
    text = b"H\t0.0.3\t.\t.\t.\nD\t0\t.\t1\t.\nF\t1\t>1>7\t3\tL\nT\t2\t>4>6\t3\tL\nC\t3\t>4>7\t.\tL\n"
    d = hl.povu_pvst_parse(text, len(text), err, 256)
    assert d, err.value
    assert [d.contents.parent[i] for i in range(4)] == [NIL, 0, NIL, 2]
    assert [d.contents.height[i] for i in range(4)] == [0, 1, 0, 2]
    hl.povu_pvst_doc_free(d)
    assert not hl.povu_pvst_parse(b"X\t1\t>1>2\t.\tL\n", 13, err, 256) and b"Unknown vertex type" in err.value
    assert not hl.povu_pvst_parse(b"T\t1\t12\t.\tL\n", 11, err, 256) and b"malformed vertex label" in err.value
    # comp_heights walks every listing (pvst.hpp:807-836): a chain of k doubly-listed diamonds takes 2^k steps, a cycle never
    # ends.  A short chain is walked out (the last visit's height stands), a long one and a cycle FAIL the parse with a message
    # instead of handing out half-filled heights
    def diamonds(k):
        rows = ["H\t0.0.3\t.\t.\t.", "D\t0\t.\t1\t."]
        for j in range(k):  # vertex 3j+1 lists 3j+2 and 3j+3, both list 3j+4
            a = 3 * j + 1
            rows += [f"F\t{a}\t>1>2\t{a + 1}, {a + 2}\tL", f"F\t{a + 1}\t>1>2\t{a + 3}\tL", f"F\t{a + 2}\t>1>2\t{a + 3}\tL"]
        rows.append(f"F\t{3 * k + 1}\t>1>2\t.\tL")
        return ("\n".join(rows) + "\n").encode()
    text = diamonds(5)
    d = hl.povu_pvst_parse(text, len(text), err, 256)
    assert d, err.value
    assert d.contents.height[d.contents.n - 1] == 11 and d.contents.parent[d.contents.n - 1] == 15
    hl.povu_pvst_doc_free(d)
    text = diamonds(40)
    assert not hl.povu_pvst_parse(text, len(text), err, 256) and b"comp_heights" in err.value
    text = b"H\t0.0.3\t.\t.\t.\nD\t0\t.\t1\t.\nF\t1\t>1>7\t2\tL\nF\t2\t>4>6\t1\tL\n"
    assert not hl.povu_pvst_parse(text, len(text), err, 256) and b"cycle" in err.value


def test_host_code_under_address_and_ub_sanitizers(golden_dir, tmp_path):
    """The tokenizer, the PVST reader and the call's host half (sites of every PVST that parses; names and the VCF writer on a
    hand-made povu_hip_calls) under -fsanitize=address,undefined (CPU build; the GPU pool has no sanitizer runs) over every
    golden input, the malformed fixtures and truncated PVST texts; before those, the wire formats of a forest on hand-made
    tables, headers and extended trees (good ones round-trip, bad ones are refused)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "povu_amd", "csrc"), "asan", "-s"])
    exe = os.path.join(root, "build", "obj", "host_asan_check")
    big = tmp_path / "chain.gfa"
    big.write_text(W.chain_of_bubbles(3000).to_gfa())
    bad = tmp_path / "bad.gfa"
    bad.write_text("S\t1\nL\t1\t+\t2\n")
    # several tokenizer slices (>= 4 MiB each), and the same text cut off inside a record at a few places: the reading of S
    # and L records front to back must stop at the end of the mapping whatever it is in the middle of
    wide = W.chain_of_bubbles(110000).to_gfa().encode()
    assert len(wide) > 4 * (4 << 20)
    cuts = []
    for k, n in enumerate((len(wide), len(wide) - 1, len(wide) - 2, len(wide) - 3, len(wide) - 5, len(wide) - 9, len(wide) // 2 + 1)):
        q = tmp_path / f"wide{k}.gfa"
        q.write_bytes(wide[:n])
        cuts.append(str(q))
    files = cuts + sorted(glob.glob(os.path.join(golden_dir, "gfa", "*.gfa")) + glob.glob(os.path.join(golden_dir, "pvst", "*.pvst")))
    r = subprocess.run([exe] + files + [str(big), str(bad)], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "parsed" in r.stdout
    assert "forest_wire ok" in r.stdout  # (the tree table, the pack / share headers and the extended trees: hip/forest_wire.hpp)
    # the PVST writer against its naive restatement and its refusals; the hooks of a pass against the table of what they gave
    # where they used to be read; every golden PVST written back from its parse, byte for byte
    assert "pvst_writer ok" in r.stdout and "pass_hooks ok" in r.stdout
    n_pvst = len(glob.glob(os.path.join(golden_dir, "pvst", "*.pvst")))
    assert n_pvst >= 13 and f"{n_pvst} written back" in r.stdout


def test_gfa_writer_is_the_inverse_of_the_loader_contract(tmp_path):
    """povu_hip_gfa_write (host only): the text equals the workload generator's own GFA text, record for record."""
    from povu_amd import hip as H, workloads as W
    for g in (W.random_bidirected(300, 520, 11, self_loops=True), W.chain_of_bubbles(50), W.hprc_shaped([120, 30], seed=2, tiny=3)):
        p = tmp_path / "g.gfa"
        H.write_gfa(g, str(p))
        assert p.read_text() == g.to_gfa()
    with pytest.raises(RuntimeError):
        H.write_gfa(W.chain_of_bubbles(3), str(tmp_path / "no" / "such" / "dir.gfa"))


def test_subtree_formatter_on_the_host():
    """povu_hip_pvst_format_subtree (write_pvst, src/mto/to_pvst.cpp:31-109, of a tree with its -s vertices): host code, no GPU.
    The tree of tests/test_oracle_subflubbles.py's hand-traced case: a concealed vertex listed under two parents."""
    from povu_amd.hip import _SubTree
    lib = C.CDLL(os.path.join(LIB, "libpovu_hip.so"))
    lib.povu_hip_pvst_format_subtree.restype = C.c_void_p
    lib.povu_hip_pvst_format_subtree.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.povu_hip_buffer_free.argtypes = [C.c_void_p]
    u8 = lambda xs: (C.c_uint8 * len(xs))(*xs)    # noqa: E731
    u32 = lambda xs: (C.c_uint32 * len(xs))(*xs)  # noqa: E731
    fam, or1, or2, route = u8(list(b"DFTC")), u8([0, 0, 0, 0]), u8([0, 0, 0, 1]), u8([0, ord("L"), ord("L"), ord("R")])
    id1, id2 = u32([0, 1, 4, 4]), u32([0, 7, 6, 7])
    off, child = u32([0, 1, 2, 3, 3]), u32([1, 3, 3])
    st = _SubTree(4, 3, 1, 0, 0, fam, or1, or2, route, id1, id2, off, child)
    n = C.c_size_t(0)
    p = lib.povu_hip_pvst_format_subtree(C.byref(st), C.byref(n))
    text = C.string_at(p, n.value).decode()
    lib.povu_hip_buffer_free(p)
    assert text == "H\t0.0.3\t.\t.\t.\nD\t0\t.\t1\t.\nF\t1\t>1>7\t3\tL\nT\t2\t>4>6\t3\tL\nC\t3\t>4<7\t.\tR\n"

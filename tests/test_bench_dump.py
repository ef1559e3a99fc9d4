"""bench.py --dump-outputs: the forest of the last timed step as .npy files.  CPU: the layout and the fixed sample of
bench.forest_outputs on a forest made up here.  GPU: the files of two runs with different --steps are the same, and
the PVST text formatted back from them is the oracle's."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle_lib as O
from povu_amd import hip as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NIL = 0xFFFFFFFF


class _FakeForest:
    """The part of hip.Forest that forest_outputs reads."""

    def __init__(self, trees):
        self.trees = trees

    def component_ids(self):
        return [t.component_id for t in self.trees]

    def pvst_sizes(self):
        return [len(t.a_id) for t in self.trees]

    def tree(self, i):
        return self.trees[i]


def _fake_forest(seed, n_trees=40):
    rng = np.random.default_rng(seed)
    trees = []
    for cid in rng.permutation(np.arange(1, 3 * n_trees, 3))[:n_trees]:  # (not in component-id order)
        n = int(rng.integers(1, 300))
        parent = np.array([NIL] + [int(rng.integers(0, k)) for k in range(1, n)], dtype=np.uint32)
        trees.append(H.PvstTree(int(cid), 2 * n, 3 * n, rng.integers(1, 1 << 31, n).astype(np.uint32),
                                rng.integers(1, 1 << 31, n).astype(np.uint32), rng.integers(0, 2, n).astype(np.uint8),
                                rng.integers(0, 2, n).astype(np.uint8), parent, np.zeros((0, 2), np.uint64)))
    return _FakeForest(trees)


def test_forest_outputs_whole_forest_in_component_order():
    f = _fake_forest(1)
    out = bench.forest_outputs(f)
    trees = sorted(f.trees, key=lambda t: t.component_id)
    assert out["tree_component_id"].tolist() == [t.component_id for t in trees]
    assert out["tree_n_vtx"].tolist() == [t.n_vtx for t in trees]
    assert out["tree_n_links"].tolist() == [t.n_links for t in trees]
    assert out["tree_n_pvst"].tolist() == [len(t.a_id) for t in trees]
    total = sum(len(t.a_id) for t in trees)
    assert out["pvst_index"].tolist() == list(range(total))
    for k in ("a_id", "z_id", "parent", "a_or", "z_or"):
        want = np.concatenate([getattr(t, k) for t in trees])
        assert out["pvst_" + k].dtype == (np.float32 if k.endswith("_or") else np.float64)
        assert np.array_equal(out["pvst_" + k], want.astype(np.float64)), k  # (exact: ids and NIL below 2^53)


def test_forest_outputs_sample_is_fixed_and_within_budget():
    f = _fake_forest(2, n_trees=200)
    full = bench.forest_outputs(f)
    total = len(full["pvst_index"])
    budget = 16 * 1024 + 32 * 200 + 40 * (total // 5)
    a, b = bench.forest_outputs(f, budget), bench.forest_outputs(_fake_forest(2, n_trees=200), budget)
    assert sum(v.nbytes for v in a.values()) <= budget
    assert len(a["pvst_index"]) == total // 5
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    idx = a["pvst_index"].astype(np.int64)
    assert np.all(np.diff(idx) > 0)
    for k in ("a_id", "z_id", "parent", "a_or", "z_or"):
        assert np.array_equal(a["pvst_" + k], full["pvst_" + k][idx]), k
    assert np.array_equal(a["tree_component_id"], full["tree_component_id"])


def _bench_dump(out, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--workload", "hprc-wg", "--scale", "0.002", "--no-secondary", "--no-cpu-baseline", "--no-latency-leg",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    return {p[:-4]: np.load(os.path.join(out, p)) for p in sorted(os.listdir(out))}


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_and_match_the_oracle(tmp_path):
    a = _bench_dump(tmp_path / "a", 1)
    b = _bench_dump(tmp_path / "b", 3)
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES
    assert a["pvst_index"].tolist() == list(range(len(a["pvst_index"])))  # (small enough to be dumped whole)
    g, _ = bench.build_workload("hprc-wg", 0.002)
    want = O.decompose(g)
    assert a["tree_component_id"].astype(np.int64).tolist() == sorted(want)
    hl = H.load_lib()
    hl.povu_hip_pvst_format.restype = C.c_void_p
    hl.povu_hip_pvst_format.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_size_t)]
    start = np.concatenate([[0], np.cumsum(a["tree_n_pvst"].astype(np.int64))])
    for j, cid in enumerate(a["tree_component_id"].astype(np.int64)):
        s = slice(start[j], start[j + 1])
        arrs = [a["pvst_a_id"][s].astype(np.uint32), a["pvst_z_id"][s].astype(np.uint32), a["pvst_a_or"][s].astype(np.uint8),
                a["pvst_z_or"][s].astype(np.uint8), a["pvst_parent"][s].astype(np.uint32)]
        ln = C.c_size_t(0)
        ptr = hl.povu_hip_pvst_format(len(arrs[0]), *[x.ctypes.data for x in arrs], C.byref(ln))
        assert ptr, cid
        got = C.string_at(ptr, ln.value).decode()
        hl.povu_hip_buffer_free(ptr)
        assert got == want[int(cid)], cid

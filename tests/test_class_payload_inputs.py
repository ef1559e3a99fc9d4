"""CPU tests of the builders behind tests/test_gpu_class_payload.py: the oracle says whether each of them makes what its name
says -- list sizes at the edges of the payload's field, valid and invalid sort entries, children counts and first-child
subtrees of the branching vertices -- and the field-width model is checked at the edges the header asserts."""
import numpy as np
import pytest

import class_payload_cases as CP
from povu_amd import workloads as W
from class_payload_cases import concat, sized_components


def test_field_width_at_its_edges():
    """lsz_field's static_asserts (par_kernels.hpp), through the model the GPU tests use."""
    assert [CP.field_width(s) for s in (1, (1 << 24) - 1, 1 << 24, (1 << 27) - 1, 1 << 27, 1 << 29, (1 << 32) - 1)] == [8, 8, 7, 5, 4, 2, 0]
    assert CP.field_width(1 << 24, 3) == 3 and CP.field_width(1 << 29, 3) == 2 and CP.field_width(5, 0) == 0
    assert [CP.lmax(w) for w in (0, 1, 2, 3, 5, 8)] == [0, 1, 3, 7, 31, 255]


@pytest.mark.parametrize("depth", range(1, 10))
def test_towers_reach_every_size_up_to_depth_plus_one(depth):
    sizes = CP.all_list_sizes(CP.towers(depth))
    assert sizes.min() == 1 and sizes.max() == depth + 1
    assert set(sizes.tolist()) == set(range(1, depth + 2))


@pytest.mark.parametrize("w", CP.WIDTHS)
def test_towers_put_both_kinds_of_boundary_under_one_width(w):
    """The tops the GPU test asks for: LMAX - 1 (nothing saturates), LMAX (one saturated size), LMAX + 1 and LMAX + 2 (two and
    three different saturated sizes, next to each other in stack order, and an unsaturated one next to LMAX when w > 1 --
    at w = 1 every size is saturated, the smallest is 1)."""
    lm = CP.lmax(w)
    for top in (lm - 1, lm, lm + 1, lm + 2):
        if top < 2:
            continue
        sizes = CP.all_list_sizes(CP.towers(top - 1))
        assert sizes.max() == top
        sat = sizes >= lm
        assert sat.any() == (top >= lm)
        steps = set(zip(sizes[:-1].tolist(), sizes[1:].tolist()))
        if top > lm:
            assert any(a >= lm and b >= lm and a != b for a, b in steps)
        if top >= lm and lm > 1:
            assert any((a >= lm) != (b >= lm) for a, b in steps)
        assert CP.saturated(CP.towers(top - 1), w) == int(sat.sum()) and CP.saturated(CP.towers(top - 1), 0) == len(sizes)


@pytest.mark.parametrize("n_valid", [16, 17, 19, 20, 21, 23, CP.TOP_GROUP, CP.FINISH_GROUP, CP.FINISH_GROUP + 1, 2 * CP.FINISH_GROUP])
def test_valid_and_invalid_entries(n_valid):
    g = CP.valid_then_invalid(n_valid)
    assert CP.n_stack(g) == n_valid and g.n_vtx == n_valid + 4 and len(CP.components(g)) == 2
    g = CP.valid_then_invalid(n_valid, invalid=())
    assert CP.n_stack(g) == n_valid == g.n_vtx
    assert CP.all_list_sizes(g).max() >= 2  # (both kinds of entry at width 1)


def test_nested_towers_40_by_3():
    g = W.nested_towers(40, 3)
    sizes = CP.all_list_sizes(g)
    assert len(sizes) == 243 and sizes.max() == 41 and CP.field_width(243) == 8
    assert CP.saturated(g, 8) == 0 and CP.saturated(g, 5) == int((sizes >= 31).sum()) == 63


def test_several_components():
    g = concat([sized_components([2, 70, 1]), CP.towers(9, 2), sized_components([1, 2]), CP.towers(4), W.chain_of_bubbles(40),
                sized_components([1]), CP.towers(8, 1)])
    cs = CP.components(g)
    assert len(cs) == 5 and all(len(d["s_st_idx"]) for d in cs)
    for w in CP.WIDTHS:
        assert 0 < CP.saturated(g, w) < CP.n_stack(g) or w == 1


def only_branching(g):
    cs = CP.components(g)
    assert len(cs) == 1
    return CP.branching_vertices(cs[0])


@pytest.mark.parametrize("children", [2, 3, 9])
def test_children_counts(children):
    assert [len(k) for _, k in only_branching(CP.broom(2, [1] * children))] == [children]
    assert [k for _, k in only_branching(CP.broom(2, [1] * children))] == [[2] * children]
    assert max(len(k) for _, k in only_branching(CP.star(children))) == children
    assert max(len(k) for _, k in only_branching(CP.star(children, 3, 1))) == children
    # the entered side branches into its black child and the two chains of `back`, the black child into `children` chains
    assert sorted(len(k) for _, k in only_branching(CP.broom(3, [2] * children, back=(1, 2)))) == sorted([3, children])


@pytest.mark.parametrize("first", [3, 4, 5])
def test_first_child_subtrees(first):
    (v, kids), = only_branching(CP.broom(2, [first, 1, 2]))
    assert kids == [2 * first, 2, 4]
    b = dict(only_branching(CP.broom(2, [first], back=(2, 1))))
    assert [1 + 2 * first, 4, 2] in b.values()
    # ... and the first child is the next vertex in both
    for g in (CP.broom(2, [first, 1, 2]), CP.broom(2, [first], back=(2, 1))):
        d = CP.components(g)[0]
        for v, _ in CP.branching_vertices(d):
            assert d["par"][v + 1] == v


def test_branching_vertex_at_the_end():
    for n in (2, 3):
        g = concat([sized_components([5, 1]), CP.branching_last(n)])
        d = CP.components(g)[-1]
        (v, kids), = CP.branching_vertices(d)
        assert kids == [2] * n and v + 2 * n == len(d["par"]) - 1  # the children are the tree's last vertices
        assert dump_last_component_is(g, d)


def dump_last_component_is(g, d):
    """d is the dump of the graph's LAST component: nothing lies behind its tree in the vertex space."""
    from test_oracle import dump_component
    c = 0
    while dump_component(g, c) is not None:
        c += 1
    last = dump_component(g, c - 1)
    return np.array_equal(last["gid"], d["gid"])


def test_empty_slots():
    g = CP.empty_slot_next_to_valid()
    assert len(CP.components(g)) == 3 and CP.n_stack(g) < g.n_vtx
    from test_oracle import dump_component
    kinds = []
    c = 0
    while True:
        d = dump_component(g, c)
        if d is None:
            break
        kinds.append(bool(len(d["s_st_idx"])))
        c += 1
    assert kinds == [False, False, True, False, False, False, True, False, True, False]

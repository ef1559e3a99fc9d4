"""GPU tests of the class sort's payload in a black-only pass: the size of a candidate-stack entry's bracket list rides above
its stack index (LszField, par_kernels.hpp), saturating at LMAX = 2^w - 1; a saturated size is looked up in the per-entry
array.  Every case runs with POVU_HIP_LSZ_FIELD = 0 (no field: every size is looked up) and with narrow fields, so that small
graphs saturate, and compares the forest, the candidate stack, its classes (as the debug hook numbers them) and next_seen
with the CPU oracle, entry by entry; the width that ran and the number of saturated entries are asserted against the model of
class_payload_cases.  The same shapes exercise the look-ups of k_top_bracket and the children sweep of k_capping."""
import pytest

import class_payload_cases as CP
import oracle_lib as O
from povu_amd import HipDecomposer, workloads as W
from povu_amd.hip import F_ALL_VERTEX_CLASSES, F_CHECK_LAMINAR
from class_payload_cases import concat, sized_components
from test_gpu_stack_lookups import check_hooks

pytestmark = pytest.mark.gpu

HOOK = "POVU_HIP_LSZ_FIELD"


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


def run_widths(hip, monkeypatch, g, widths=(0,) + CP.WIDTHS + (None,), n_decomposed=None, black_only=True):
    """One upload; a pass per hook value (None: the hook unset), each checked against the oracle through the forest and the
    structure hooks, with the width and the saturation counter it reports.  black_only = None: the literal hi_2 rule may
    send the graph through the all-vertices pass, which has no field."""
    want = O.decompose(g)
    sizes = CP.all_list_sizes(g)
    hip.upload(g)
    for w in widths:
        if w is None:
            monkeypatch.delenv(HOOK, raising=False)
        else:
            monkeypatch.setenv(HOOK, str(w))
        ran = min(CP.field_width(len(sizes)), CP.FIELD_CAP if w is None else w)
        for fl in (0, F_CHECK_LAMINAR):
            assert hip.decompose(flags=fl).texts() == want, (w, fl)
            assert hip.last_black_only_classes() or black_only is None, (w, fl)
            model = (ran, int((sizes >= CP.lmax(ran)).sum())) if hip.last_black_only_classes() else (0, 0)
            assert hip.last_lsz_field() == model, (w, fl)
        checked = check_hooks(hip, g)
        assert checked == (len(CP.components(g)) if n_decomposed is None else n_decomposed), w
        assert hip.decompose(flags=F_ALL_VERTEX_CLASSES).texts() == want, w
        assert hip.last_lsz_field() == (0, 0), w
    monkeypatch.delenv(HOOK, raising=False)


@pytest.mark.parametrize("w", CP.WIDTHS)
def test_sizes_around_the_fields_limit(hip, monkeypatch, w):
    """Nested bubbles whose deepest list has LMAX - 1, LMAX and LMAX + 1 brackets, and one level more (two different
    saturated sizes next to each other under the bracket that spans a tower, and a saturated next to an unsaturated one)."""
    for top in (CP.lmax(w) - 1, CP.lmax(w), CP.lmax(w) + 1, CP.lmax(w) + 2):
        if top >= 2:
            run_widths(hip, monkeypatch, CP.towers(top - 1), widths=(0, w))


@pytest.mark.parametrize("n_valid", [16, 17, 19, 20, 21, 23])
def test_valid_runs_of_every_length_mod_four_in_front_of_invalid_entries(hip, monkeypatch, n_valid):
    """4m, 4m + 1 and 4m + 3 valid sorted entries followed by NIL keys (segments of components that are not decomposed), and
    by nothing: the tail lanes of k_class_finish_black and its neighbour loads at q0 - 1 and q0 + 4."""
    run_widths(hip, monkeypatch, CP.valid_then_invalid(n_valid), n_decomposed=2)
    run_widths(hip, monkeypatch, CP.valid_then_invalid(n_valid, invalid=()), widths=(0, 1), n_decomposed=2)


@pytest.mark.parametrize("n_valid", [CP.TOP_GROUP, CP.FINISH_GROUP, 2 * CP.FINISH_GROUP])
def test_valid_run_ends_on_a_workgroup_edge(hip, monkeypatch, n_valid):
    run_widths(hip, monkeypatch, CP.valid_then_invalid(n_valid), widths=(0, 1, None), n_decomposed=2)
    run_widths(hip, monkeypatch, CP.valid_then_invalid(n_valid + 1, invalid=(2,)), widths=(0, 1), n_decomposed=2)


def test_several_components_with_saturated_sizes_in_each(hip, monkeypatch):
    """The stack offsets of the components are not zero, undecomposed components lie between them, and the towers are deep
    enough to saturate every width of the tests."""
    g = concat([sized_components([2, 70, 1]), CP.towers(9, 2), sized_components([1, 2]), CP.towers(4), W.chain_of_bubbles(40),
                sized_components([1]), CP.towers(8, 1)])
    run_widths(hip, monkeypatch, g)


def test_nested_towers_40_by_3(hip, monkeypatch):
    """The default width: 243 entries leave all eight bits, so nothing of depth 40 saturates; with five bits (LMAX = 31, what a
    stack of 2^26 entries leaves) the levels from 31 on do."""
    g = W.nested_towers(40, 3)
    assert CP.field_width(CP.n_stack(g)) == CP.FIELD_CAP and CP.saturated(g, 8) == 0 and CP.saturated(g, 5) > 0
    run_widths(hip, monkeypatch, g, widths=(None, 5, 0))


def test_random_graphs_at_every_width(hip, monkeypatch):
    """Forty small connected random graphs: those that take the black-only pass report the width and the saturated entries
    of the model at every width, and the debug hook numbers their classes as the oracle does; some of them must take it."""
    black = 0
    for seed in range(40):
        g = CP.random_connected(seed)
        want = O.decompose(g)
        hip.upload(g)
        for w in (0, 1, 2, 3):
            monkeypatch.setenv(HOOK, str(w))
            assert hip.decompose().texts() == want, (seed, w)
            if hip.last_black_only_classes():
                black += 1
                assert hip.last_lsz_field() == (w, CP.saturated(g, w)), (seed, w)
            else:
                assert hip.last_lsz_field() == (0, 0), (seed, w)
            if w in (0, 2):
                assert check_hooks(hip, g) == 1, (seed, w)
    monkeypatch.delenv(HOOK, raising=False)
    assert black >= 4, black


# ---- the shapes of the look-ups of k_top_bracket and of the children sweep of k_capping
@pytest.mark.parametrize("children", [2, 3, 9])
def test_branching_vertices(hip, monkeypatch, children):
    for g in (CP.star(children), CP.star(children, 3, 1), CP.broom(2, [1] * children), CP.broom(3, [2] * children, back=(1, 2))):
        run_widths(hip, monkeypatch, g, widths=(0, 2, None), black_only=None)


@pytest.mark.parametrize("first", [3, 4, 5])
def test_first_child_around_eight_vertices(hip, monkeypatch, first):
    """The first child's subtree ends at, one before and one behind the eight words that follow the branching vertex: 2 *
    first vertices under a gray first child, 1 + 2 * first under the black one."""
    run_widths(hip, monkeypatch, CP.broom(2, [first, 1, 2]), widths=(0, 2, None), black_only=None)
    run_widths(hip, monkeypatch, CP.broom(2, [first], back=(2, 1)), widths=(0, 2, None), black_only=None)


def test_branching_vertex_at_the_end_of_the_last_tree(hip, monkeypatch):
    for n in (2, 3):
        run_widths(hip, monkeypatch, concat([sized_components([5, 1]), CP.branching_last(n)]), widths=(0, 2, None), black_only=None)


def test_empty_slots_next_to_valid_vertices(hip, monkeypatch):
    run_widths(hip, monkeypatch, CP.empty_slot_next_to_valid(), black_only=None)

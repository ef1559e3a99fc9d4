"""The minimal, empty and wide-id inputs (tests/edge_cases.py) reach the state the GPU tests put them through for, on the
restatements and the CPU oracle alone.  No GPU."""
import functools

import pytest

import edge_cases as E
import inversions_ref as I
import merge_ref as MR
import nested_ref as N
import norm_ref as NR
import offref_ref as F
import oracle_lib as O
import prim_ref as PR
import test_merge_writer as TMW
import traversals_ref as TR
import vcf_ref as V
from test_nested_ref import _vcf
from test_vcf_writer import DATE, lib  # noqa: F401  (lib: the fixture)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(case, sites, traversals of every site, plain records and (inversion records, statistics) per prefix list)."""
    case = E.MINIMAL[name]() if name in E.MINIMAL else E.wide_cases()[name][1]
    sites = V.sites_of_pvst(list(O.decompose(case.g).values()))
    flat = TR.flat(TR.PathIndex(case.steps), [(s["s"], s["z"]) for s in sites])
    calls = [V.call(sites, case.names, case.steps, case.sq, refs, case.max_steps) for refs in case.refs]
    invs = [I.records(case.names, case.steps, case.sq, refs, case.max_steps) for refs in case.refs]
    return case, sites, flat, calls, invs


def alleles_per_site(flat):
    return [int(b) - int(a) for a, b in zip(flat["allele_off"][:-1], flat["allele_off"][1:])]


def runs_of(case, refs):
    return I.runs(case.steps, V.ref_paths(case.names, refs), case.max_steps)[0]


# ---- zero and one

def test_no_sites():
    case, sites, flat, (call,), ((inv, stats),) = restated("no_sites")
    assert case.g.n_vtx == 5 and len(sites) == 0 and len(flat["path"]) == 0 and call == []
    assert (stats["heads"], stats["records"], stats["long"]) == (1, 1, 0) and inv[0]["n_steps"] == 5
    assert [r["vartype"] for r in I.merge(call, inv)] == ["SUBR"]  # inversion records without a flubble record


def test_no_sites_wide():
    case, sites, flat, (call,), ((inv, stats),) = restated("no_sites_wide")
    assert len(sites) == 0 and call == [] and (stats["heads"], stats["records"]) == (1, 1)
    assert inv[0]["at"] == [">7>1000000>99999999>2147483648>4294967294", "<4294967294<2147483648<99999999<1000000<7"]


def test_untouched_sites():
    case, sites, flat, (call,), ((inv, stats),) = restated("untouched_sites")
    assert len(O.decompose(case.g)) == 2 and len(sites) == 3 and len(flat["path"]) == 0 and call == []
    assert (stats["heads"], stats["records"]) == (1, 1)


def test_all_agree():
    case, sites, flat, (call,), ((inv, stats),) = restated("all_agree")
    assert len(sites) == 3 and len(flat["path"]) == 9 and alleles_per_site(flat) == [1, 1, 1] and call == []
    assert stats["heads"] == 0 and stats["max_opposite"] == 0


def test_uncallable():
    case, sites, flat, (call,), _ = restated("uncallable")
    assert len(sites) == 3 and min(alleles_per_site(flat)) >= 2 and call == []
    ref = case.steps[0]
    assert not any(V.called_sites(sites, {0: ref}))
    assert all(not ({s["s"][0], s["z"][0]} <= {x for x, _ in ref}) for s in sites)  # it reaches no site's second boundary
    want, counts = F.call(sites, case.names, case.steps, case.sq, case.refs[0])
    assert len(want) == 3 and all(r["offref"] for r in want) and counts["n_offref_sites"] == counts["n_offref_records"] == 3
    assert all(r["path"] != 0 for r in want)  # surrogates only


def test_one_path():
    case, sites, flat, (call,), ((inv, stats),) = restated("one_path")
    samples, slot, sample_of = V.slots_of(case.names)
    assert len(case.names) == len(samples) == len(sample_of) == 1
    assert len(flat["path"]) == 3 and call == [] and inv == [] and stats["heads"] == 0


def test_self_inverting():
    case, sites, flat, (call,), ((inv, stats),) = restated("self_inverting")
    assert len(case.names) == 1 and stats["max_opposite"] >= 1 and stats["heads"] == 0 and inv == [] and call == []
    steps = case.steps[0]
    assert {(6, 0), (6, 1), (5, 0), (5, 1)} <= set(steps)


def test_single_snp():
    case, sites, flat, (one, two), invs = restated("single_snp")
    assert case.g.n_vtx == 4 and case.seqs[1:3] == ["C", "G"] and len(sites) == 1 and len(case.names) == 2
    assert len(one) == 1 and len(two) == 2 and {r["path"] for r in two} == {0, 1}
    assert (one[0]["ref"], one[0]["alts"], one[0]["vartype"]) == ("C", ["G"], "SUB")
    assert all(stats["heads"] == 0 for _, stats in invs)


def test_runs_of_one():
    case, sites, flat, (call,), ((inv, stats),) = restated("runs_of_one")
    runs = runs_of(case, case.refs[0])
    assert stats["heads"] == len(runs) == 3 and {n for _, _, n, _, _ in runs} == {1} and inv == [] and stats["records"] == 0


def test_runs_too_long():
    case, sites, flat, (call,), ((inv, stats),) = restated("runs_too_long")
    assert case.max_steps == 2 and stats["heads"] == stats["long"] == 2 and inv == [] and stats["records"] == 0
    # without the limit they are runs of three steps, and records
    runs = I.runs(case.steps, [0])[0]
    assert [n for _, _, n, _, _ in runs] == [3, 3] and I.records(case.names, case.steps, case.sq, case.refs[0])[1]["records"] == 2


def test_baseless_runs():
    case, sites, flat, (call,), ((inv, stats),) = restated("baseless_runs")
    runs = runs_of(case, case.refs[0])
    assert stats["heads"] == 2 and sorted(n for _, _, n, _, _ in runs) == [2, 3] and stats["long"] == 0
    assert all(case.sq[x[0]] == "" for r, i, n, _, _ in runs for x in case.steps[r][i:i + n])
    assert inv == [] and stats["records"] == 0 and len(call) == 2


def test_all_empty_sequences():
    case, sites, flat, (call,), ((inv, stats),) = restated("all_empty_sequences")
    assert set(case.seqs) == {""} and len(sites) == 1
    assert len(call) == 1 and (call[0]["ref"], call[0]["alts"], call[0]["pos"]) == ("", [""], 0)  # (anchored on a base that is not there)
    assert sum(len(case.sq[x]) for x, _ in case.steps[0]) == 0  # a contig of length 0
    assert (stats["heads"], stats["records"]) == (1, 0) and inv == []


def test_empty_allele_among_others():
    case, sites, flat, (call,), _ = restated("empty_allele_among_others")
    assert len(call) == 1 and (call[0]["ref"], sorted(call[0]["alts"]), call[0]["vartype"]) == ("AC", ["", "AG"], "DEL")
    want, counters = NR.normalise(call, case.steps, case.sq)
    assert counters == dict(n_normalized=0, max_shift=0, n_norm_compared=0) and not want[0]["normalized"]
    # the two texts that are there differ in their last base: compared on their own they would count a position
    assert NR.closed_form("GG", ["AC", "AG"])[4] == 1


def test_popped_drops_all():
    case, sites, flat, (call,), _ = restated("popped_drops_all")
    args = (sites, case.names, case.steps, case.sq, case.refs[0])
    nested = N.call(*args)
    assert len(nested) == 1 and len(nested[0]["ref"]) == 8 > case.popped["max_ref_length"] == 1
    popped, counters = N.call_full(*args, profile="popped", **case.popped)
    assert popped == [] and counters["n_popped"] == 1 and counters["n_rescued"] == 0


@pytest.mark.parametrize("second", [False, True])
def test_zero_step_paths(second):
    case = E.zero_step_paths(second)
    lens = [len(st) for st in case.steps]
    assert [k for k, n in enumerate(lens) if n == 0] == [0, 3, 5] and len(lens) == 6
    refs = V.ref_paths(case.names, case.refs[0])
    assert refs == ([1, 3] if second else [1])
    sites = V.sites_of_pvst(list(O.decompose(case.g).values()))
    call = V.call(sites, case.names, case.steps, case.sq, case.refs[0])
    assert len(call) == 3 and {r["path"] for r in call} == {1}
    # the paths without a step have a column of their own, and no call in it
    assert all(len(r["slots"]) == 6 and [r["slots"][k] for k in (0, 3, 5)] == [None] * 3 for r in call)
    inv, stats = I.records(case.names, case.steps, case.sq, case.refs[0])
    assert stats["records"] == len(inv) == 1 and inv[0]["slots"][4] == 1  # the haplotype behind the second empty path


def test_one_step_paths():
    case, sites, flat, (call,), ((inv, stats),) = restated("one_step_paths")
    ref = case.steps[0]
    ones = [st[0] for st in case.steps if len(st) == 1]
    assert len(ones) == 6 and sum(TR.flip(s) in ref for s in ones) == 4 and TR.flip(ref[0]) in ones and TR.flip(ref[-1]) in ones
    runs = runs_of(case, case.refs[0])
    assert stats["heads"] == 4 and {n for _, _, n, _, _ in runs} == {1} and inv == [] and len(call) == 3


def test_one_vertex():
    case, sites, flat, (call,), ((inv, stats),) = restated("one_vertex")
    assert case.g.n_vtx == 1 and case.g.n_links == 0 and case.steps == [[(5, 0)], [(5, 1)]]
    assert sites == [] and call == [] and (stats["heads"], stats["records"]) == (1, 0)


def test_every_minimal_case_is_small_and_has_a_test():
    for name, make in E.MINIMAL.items():
        assert make().g.n_vtx <= 300 and "test_" + name in globals(), name


# ---- wide ids

@pytest.mark.parametrize("v", [16, 17, 72, 112, 133, 300, 901, 1201])
def test_wide_ids(v):
    ids = E.wide_ids(v).tolist()
    assert len(ids) == v and ids == sorted(set(ids)) and {len(str(i)) for i in ids} == set(range(1, 11))
    assert {1, 2147483647, 2147483648, 4294967294} <= set(ids)
    assert sum(i < 2 ** 31 - 1 for i in ids if len(str(i)) == 10) >= 1 and sum(2 ** 31 < i < 4294967294 for i in ids) >= 1


def test_relabel_keeps_the_graph_and_the_paths():
    for name in E.WIDE:
        plain, wide, ids = E.wide_cases()[name]
        m = E.id_map(plain.g, ids)
        assert wide.g.vid.tolist() == ids.tolist() and all(getattr(wide.g, k) is getattr(plain.g, k) or
                                                           (getattr(wide.g, k) == getattr(plain.g, k)).all() for k in ("v1", "s1", "v2", "s2"))
        assert wide.steps == [[(m[i], o) for i, o in st] for st in plain.steps] and wide.names == plain.names and wide.seqs == plain.seqs


@pytest.mark.parametrize("name", E.WIDE)
def test_wide_case(name):
    case, sites, flat, calls, invs = restated(name)
    recs = [r for call, (inv, _) in zip(calls, invs) for r in call + inv]
    in_at = {i for r in recs for a in r["at"] for i in E.ids_of_at(a)}
    assert {len(str(i)) for i in in_at} == set(range(1, 11))
    assert max(in_at) >= 2 ** 31 and min(i for i in in_at if len(str(i)) == 10) < 2 ** 31  # compared on both sides
    assert any(i >= 2 ** 31 for st in case.steps for i, _ in st)
    called = {r["id"] for call in calls for r in call}
    assert any(max(s["s"][0], s["z"][0]) >= 2 ** 31 for s in sites if V.label(s["s"], s["z"]) in called)
    assert any(r["vartype"] == "SUBR" for r in recs) and any(r["vartype"] != "SUBR" for r in recs)


def test_long_allele_and_long_run():
    case, sites, flat, (call,), ((inv, stats),) = restated("long")
    long = [r for r in call if max(len(E.ids_of_at(a)) for a in r["at"]) >= 65]
    assert len(long) == 1 and [len(E.ids_of_at(a)) for a in long[0]["at"]] == [E.LONG, 1, E.LONG]  # (the first segment is no anchor: a SUB)
    assert all(len(str(i)) == 10 for a in long[0]["at"] for i in E.ids_of_at(a))
    assert [r["n_steps"] for r in inv] == [E.LONG] and stats["tier2"] == 1
    assert all(len(str(i)) == 10 for i in E.ids_of_at(inv[0]["at"][0]))
    # the second round of 64 steps begins behind 64 steps of 11 bytes each
    assert long[0]["at"][0].index(">" + str(E.ids_of_at(long[0]["at"][0])[64])) == 64 * 11


# ---- the host writer on a merged call without a row

def test_writer_names_the_merge_fields_of_a_call_without_a_row(lib):
    """A call made with the merge flag that ends without a record has no array to show for it (the library hands NULL): its
    header still names MERGED and MERGED_FROM, as the restatement's does."""
    case = E.all_agree()
    names, steps, sq = case.names, case.steps, case.sq
    raw, rows, merged, pack, sites, nr = TMW._case(lib, names, steps, sq, list(O.decompose(case.g).values()), case.refs[0])
    assert raw == [] and rows == [] and merged == []
    calls, keep = pack()
    for k, t in TMW._FIELDS.items():
        if isinstance(getattr(calls, k), t) and k != "contig_len":
            setattr(calls, k, None)
    got = _vcf(lib, calls, sites, nr, names, PR.PROFILE)
    assert got == MR.vcf_text(names, steps, sq, raw, rows, merged, case.refs[0], date=DATE) and got.count("##INFO=<ID=MERGED") == 2
    calls.merged = 0  # without the flag: the decomposed profile's header
    assert _vcf(lib, calls, sites, nr, names, PR.PROFILE) == PR.vcf_text(names, steps, sq, raw, rows, case.refs[0], date=DATE)
    del keep
    lib.povu_hip_call_names_free(nr)

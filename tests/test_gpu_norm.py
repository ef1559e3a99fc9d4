"""GPU left-normalised calls (povu_hip_call_profile under POVU_HIP_PROFILE_LEFT_NORMALIZED, `povu call --profile
left-normalized`) against the plain-Python restatement (tests/norm_ref.py), array for array and VCF text for VCF text,
exactly: the reference's fixture through the library, the CLI and gfa2vcf; hand-built chains that put the end of a repeat
on and around the 64-base chunk of the backward walk, cut the context into one-base and long segments, cross it with '-'
steps, lower case and a reference path that walks the graph backwards, begin the contig with the repeat, give a record
several ALTs, chop and trim without a shift and make two records swap places; the nested call, the inversion records and
the forced second tier beside it; graphs that must stay as they are; tandem_indels against the restatement;
the wide cohort of 131 samples in 261 slots (tests/cohort_cases.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import cohort_cases as CC
import inversions_ref as I
import nested_ref as N
import norm_ref as NR
import vcf_ref as V
from povu_amd import HipDecomposer
from povu_amd import hip as H
from povu_amd import workloads as W
from test_oracle import _load_gfa_links

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POVU = os.path.join(ROOT, "povu_amd", "bin", "povu")
DATE = "00000000"
NIL = 0xFFFFFFFF
FIXTURE = "downstream_repetitive/tandem-repeat-left-normalization"
VCFWAVE = "downstream_repetitive/vcfwave-complex-decomposition"
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


@pytest.fixture(scope="module")
def hip():
    d = HipDecomposer(0)
    yield d
    d.close()


# ---- hand-built chains
def chain(items, haps, reversed_copy=False):
    """(graph, sequences, paths) of a chain.  items: ("s", text, rev) a segment every haplotype walks (stored reverse-complemented
    and walked '-' when rev), ("b", [text, ...], skippable) a bubble of parallel segments.  haps: per haplotype its choice at
    every bubble, in order (0: the skip link, k: segment k).  With reversed_copy one more path walks haplotype 0 backwards."""
    seqs, plan = [], []
    for it in items:
        if it[0] == "s":
            seqs.append(it[1].encode().translate(_RC)[::-1].decode() if it[2] else it[1])
            plan.append((len(seqs), it[2]))
        else:
            ids = []
            for t in it[1]:
                seqs.append(t)
                ids.append(len(seqs))
            plan.append(ids)
    walks = []
    for choice in haps:
        st, b = [], 0
        for p in plan:
            if isinstance(p, tuple):
                st.append(p)
            else:
                if choice[b]:
                    st.append((p[choice[b] - 1], 0))
                b += 1
        walks.append(st)
    names = [f"hap{k}#1#chr1" for k in range(len(walks))]
    if reversed_copy:
        walks.append([(i, 1 - r) for i, r in reversed(walks[0])])
        names.append("back#1#chr1")
    seen, v1, s1, v2, s2 = set(), [], [], [], []
    for st in walks[:len(haps)]:
        for a, b in zip(st, st[1:]):
            if (a, b) not in seen:
                seen.add((a, b))
                v1.append(a[0] - 1), s1.append(W.L if a[1] else W.R), v2.append(b[0] - 1), s2.append(W.R if b[1] else W.L)
    g = W._mk(np.arange(1, len(seqs) + 1), v1, s1, v2, s2)
    return g, seqs, W._paths(names, [([i for i, _ in st], [r for _, r in st]) for st in walks])


def cut(text, long_at=None, long_len=0, rev_every=0, lower_every=0):
    """`text` as one-base segments, but one of long_len bases from long_at; every rev_every-th walked '-', every lower_every-th
    lower case."""
    out, at, k = [], 0, 0
    while at < len(text):
        ln = long_len if at == long_at else 1
        piece = text[at:at + ln]
        at += len(piece)
        k += 1
        if lower_every and k % lower_every == 0:
            piece = piece.lower()
        out.append(("s", piece, int(bool(rev_every) and k % rev_every == 0 and at < len(text))))
    return out


def boundary_items():
    """Twelve units: a flank that ends in G, a repeat of 63, 64, 65 or 129 bases of period 1, 2 or 3 that begins with a partial
    period, an indel of one period at its right end."""
    items = []
    for total in (63, 64, 65, 129):
        for motif in ("A", "CA", "CTA"):
            text = (motif * (total // len(motif) + 1))[-total:]
            items += [("s", "TCTG", 0)]
            items += cut(text, 20, 70, rev_every=7, lower_every=5) if total == 129 else cut(text, 9, 30, rev_every=5, lower_every=11)
            items += [("b", [motif], True)]
    return items + [("s", "GT", 0)]


def _setup(d, g, seqs, paths, flags=0):
    d.upload(g)
    f = d.decompose(flags=flags)
    d.upload_paths(paths)
    d.upload_sequences(seqs)
    steps = [paths.steps(k) for k in range(len(paths))]
    sq = dict(zip(g.vid.tolist(), seqs))
    sites = V.sites_of_pvst([f.text(i) for i in range(len(f))])
    return f, sites, list(paths.names), steps, sq


def _text_of(c, k):
    return bytes(c.seq[int(c.seq_off[k]):int(c.seq_off[k + 1])]).decode()


def _same(c, want, counters):
    n = len(want)
    assert c.n_records == n
    assert [(int(c.path[i]), int(c.pos[i]), int(c.query[i]), int(c.first[i])) for i in range(n)] == \
        [(r["path"], r["pos"], r["q"], r["first"]) for r in want]
    assert c.raw_pos.tolist() == [r["raw_pos"] for r in want]
    assert c.norm_shift.tolist() == [r["s"] for r in want] and c.norm_chop.tolist() == [r["r"] for r in want]
    assert c.norm_trim.tolist() == [r["u"] for r in want]
    assert [bool(x & H.CALL_NORMALIZED) for x in c.flags.tolist()] == [r["normalized"] for r in want]
    assert [int(b) != NIL for b in c.norm_block.tolist()] == [r["normalized"] for r in want]
    for i, r in enumerate(want):
        assert _text_of(c, int(c.ref_spelled[i])) == r["raw_ref"]
        if r["normalized"]:
            b = int(c.block_off[c.norm_block[i]])
            assert int(c.block_off[c.norm_block[i] + 1]) - b == int(c.n_alleles[i]) == 1 + len(r["alts"])
            assert [_text_of(c, b + k) for k in range(1 + len(r["alts"]))] == [r["ref"]] + r["alts"]
            assert int(c.at_off[b]) == int(c.at_off[b + 1 + len(r["alts"])])
    assert dict(n_normalized=c.n_normalized, max_shift=c.max_shift, n_norm_compared=c.n_norm_compared) == counters


def _check(d, setup, prefixes, tflags=0):
    """The call under the profile equals the restatement; returns (calls, its records, its counters)."""
    f, sites, names, steps, sq = setup
    nested = bool(tflags & H.T_NESTED)
    raw = N.call(sites, names, steps, sq, prefixes) if nested else V.call(sites, names, steps, sq, prefixes)
    line = N.record_line if nested else V.record_line
    if tflags & H.T_INVERSIONS:
        raw = I.merge(raw, I.records(names, steps, sq, prefixes)[0])
        flubble_line = line  # (inversions_ref writes a flubble record as vcf_ref does: a nested one keeps nested_ref's line)
        line = lambda r: I.record_line(r) if r["vartype"] == "SUBR" else flubble_line(r)  # noqa: E731
    want, counters = NR.normalise(raw, steps, sq)
    c = d.call(f, prefixes, flags=tflags, profile=NR.PROFILE)
    assert c.nested == nested
    _same(c, want, counters)
    assert c.vcf_text(date=DATE) == NR.vcf_text(names, steps, sq, want, prefixes, raw_line=line, date=DATE, nested=nested)
    return c, want, counters


# ---- the fixture
def _fixture_setup(d, golden_dir, name):
    gfa = os.path.join(golden_dir, "gfa", name + ".gfa")
    names, paths, seqs = V.read_gfa(gfa)
    g = _load_gfa_links(gfa)
    p = W._paths(names, [([i for i, _ in st], [r for _, r in st]) for st in paths])
    return _setup(d, g, [seqs[i] for i in g.vid.tolist()], p)


def test_fixture_through_the_library(hip, golden_dir):
    want = json.load(open(os.path.join(golden_dir, "reference_norm_records.json")))
    c, recs, counters = _check(hip, _fixture_setup(hip, golden_dir, FIXTURE), ["HG1"])
    (r,), w0 = recs, want["records"][0]
    assert (r["chrom"], r["pos"], r["id"], r["ref"], r["alts"], r["raw_pos"]) == (w0["chrom"], w0["pos"], w0["id"], w0["ref"], ["A", "AAA"], 4)
    assert (r["r"], r["s"], r["u"]) == (3, 3, 0) and counters == dict(n_normalized=1, max_shift=3, n_norm_compared=11)
    line = c.vcf_text(date=DATE).splitlines()[-1]
    assert line.startswith("HG1#1#chr1\t1\t>3>5:norm\tAA\tA,AAA\t60\tPASS\t")
    assert line.endswith(";ES=>3>5;LV=0;ORIGIN=>3>5;RAW_ALT_INDEX=1,2;PROFILE=left-normalized;LEFT_NORMALIZED=T;RAW_POS=4;RAW_REF=AA;"
                         "RAW_ALT=A,AAA\tGT\t0\t1\t2")
    info = dict(kv.split("=", 1) for kv in line.split("\t")[7].split(";"))
    assert {k: info[k] for k in w0["info"]} == dict(w0["info"], RAW_ALT_INDEX="1,2", RAW_ALT="A,AAA")
    assert (info["AT"].split(",")[:2], info["VARTYPE"]) == (w0["at"], w0["vartype"])  # (traversal provenance and VARTYPE stay raw)


def test_fixture_through_the_cli_and_gfa2vcf(golden_dir, tmp_path):
    gfa = os.path.join(golden_dir, "gfa", FIXTURE + ".gfa")
    out = tmp_path / "forest"
    out.mkdir()
    r = subprocess.run([POVU, "decompose", "-i", gfa, "-o", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    names, paths, seqs = V.read_gfa(gfa)
    sites = V.sites_of_pvst([(out / "1.pvst").read_text()])
    raw = V.call(sites, names, paths, seqs, ["HG1"])
    recs, _ = NR.normalise(raw, paths, seqs)
    want = NR.vcf_text(names, paths, seqs, recs, ["HG1"], date=DATE).split("\n", 2)[2]
    for cmd in ([POVU, "call", "-i", gfa, "-f", str(out), "-P", "HG1", "--profile", "left-normalized"],
                [POVU, "call", "-i", gfa, "-f", str(out), "-P", "HG1", "--profile=left-normalized", "--max-level", "3", "--max-ref-length=1"],
                [POVU, "gfa2vcf", "-i", gfa, "-P", "HG1", "--stdout", "--profile=left-normalized"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, POVU_CALL_EXE=POVU))
        assert r.returncode == 0, r.stderr
        assert r.stdout.split("\n", 2)[2] == want, cmd  # (behind the date line)
    assert "\t1\t>3>5:norm\tAA\tA,AAA\t" in want and "##INFO=<ID=PS," not in want  # (the profile does not imply --nested)
    # without the profile: the raw call, byte for byte
    r = subprocess.run([POVU, "call", "-i", gfa, "-f", str(out), "-P", "HG1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split("\n", 2)[2] == V.vcf_text(names, paths, seqs, raw, ["HG1"], date=DATE).split("\n", 2)[2]


# ---- chunk and step boundaries, orientation
def test_repeat_ends_around_the_chunk_boundary(hip):
    items = boundary_items()
    nb = sum(1 for it in items if it[0] == "b")
    haps = [[k % 2 for k in range(nb)], [1 - k % 2 for k in range(nb)], [1] * nb]
    g, seqs, p = chain(items, haps)
    setup = _setup(hip, g, seqs, p)
    c, want, counters = _check(hip, setup, ["hap0"])
    # every unit's indel goes to the left end of its repeat: the G of the flank is the anchor
    assert [r["s"] for r in want] == [t for t in (63, 64, 65, 129) for _ in range(3)] and counters["n_normalized"] == nb
    assert all(r["ref"][0] == "G" and r["alts"][0][0] == "G" and r["u"] == 0 for r in want)
    assert {r["vartype"] for r in want} == {"INS", "DEL"}
    # what the cut reaches, on the input: '-' steps, lower case, one-base segments, a segment longer than a chunk
    assert any(r for _, r in setup[3][0]) and any(s != s.upper() for s in seqs) and max(map(len, seqs)) == 70 and seqs.count("A") > 100
    c2, _, _ = _check(hip, setup, ["hap0"], tflags=H.T_FORCE_TIER2)
    assert c2.vcf_text(date=DATE) == c.vcf_text(date=DATE)


def test_reference_that_walks_the_graph_backwards(hip):
    # flank, bubble, repeat: for the path that walks the chain backwards the repeat lies in front of the site, which it crosses
    # from its exit to its entry
    items = []
    for total, motif in ((64, "A"), (65, "CA"), (70, "CTA")):
        text = (motif * (total // len(motif) + 1))[:total]
        items += [("s", "TCTG", 0), ("b", [motif], True)] + cut(text, 9, 30, rev_every=4, lower_every=6) + [("s", "G", 0)]
    g, seqs, p = chain(items, [[1, 0, 1], [0, 1, 0], [1, 1, 1]], reversed_copy=True)
    setup = _setup(hip, g, seqs, p)
    c, want, counters = _check(hip, setup, ["back"])
    assert sorted(r["s"] for r in want) == [64, 65, 70] and all(r["normalized"] for r in want)
    # both references in one call: two paths, each with its own context
    c, want, counters = _check(hip, setup, ["hap0", "back"])
    assert len({r["path"] for r in want}) == 2 and counters["max_shift"] == 70


def test_contig_start_multi_alt_chop_trim_and_order(hip):
    items = [("s", "A", 0)] * 4 + [("b", ["A"], True)]                      # the repeat begins at base 1: the cap
    items += [("s", "CGT", 0)] + [("s", "A", 0)] * 6 + [("b", ["A", "CA"], True)]   # two ALTs that limit r differently
    items += [("s", "CGT", 0)] + [("s", "A", 0)] * 6 + [("b", ["A", "A"], True)]    # an ALT with REF's text
    items += [("s", "CG", 0), ("b", ["TCA", "GA"], False)]                  # a common suffix only
    items += [("s", "CG", 0), ("b", ["ACT", "AG"], False)]                  # a common prefix only
    items += [("s", "CG", 0), ("b", ["ACTA", "ACGA", "ACGGA"], False)]      # both, three alleles
    items += [("s", "G", 0)] + [("s", "A", 0)] * 8 + [("b", ["A", "G"], False)] + [("s", "A", 0)] * 5 + [("b", ["A"], True)]  # a swap
    items += [("s", "CT", 0)]
    haps = [[0, 0, 1, 1, 1, 1, 1, 1], [1, 1, 2, 2, 2, 2, 2, 0], [1, 2, 0, 1, 2, 3, 1, 0], [0, 0, 1, 1, 1, 2, 1, 1]]
    g, seqs, p = chain(items, haps)
    setup = _setup(hip, g, seqs, p)
    for tflags in (0, H.T_NESTED):
        c, want, counters = _check(hip, setup, ["hap0"], tflags=tflags)
        by = {r["raw_pos"]: r for r in want}
        first = want[0]
        assert (first["pos"], first["raw_pos"], first["ref"], first["alts"], first["s"]) == (1, 4, "A", ["AA"], 3)
        multi = [r for r in want if len(r["alts"]) == 2 and r["s"] == 1]
        assert len(multi) == 1 and multi[0]["r"] == 1
        same = [r for r in want if r["raw_ref"] in r["raw_alts"]]  # an ALT with REF's text: the shift ends at the repeat's left end
        assert len(same) == 1 and same[0]["s"] == 6 and same[0]["pos"] > 8
        assert [(r["raw_ref"], r["ref"], r["alts"], r["s"], r["u"], r["pos"] - r["raw_pos"]) for r in want if r["vartype"] == "SUB"][:3] == [
            ("TCA", "TC", ["G"], 0, 0, 0), ("ACT", "CT", ["G"], 0, 1, 1), ("ACTA", "T", ["G", "GG"], 0, 2, 2)]
        assert len(by) == len(want)
        pos, raw_pos = c.pos.tolist(), c.raw_pos.tolist()
        assert pos == sorted(pos) and raw_pos != sorted(raw_pos)  # two records swapped places


# ---- composition
def test_nested_call_on_skip_nested_with_homopolymer_spacers(hip):
    units, depth = 12, 1
    g = W.skip_nested(units, depth, seed=1)
    p = W.pansn(W.skip_haplotypes(units, depth, 8, seed=1), samples=4)
    _, snp, _, _, _ = W._skip_template(depth, 2)
    seqs = ["A" if s[0] < 0 else "CG"[s[1]] for s in snp] * units
    setup = _setup(hip, g, seqs, p)
    c, want, counters = _check(hip, setup, ["sample0#1"], tflags=H.T_NESTED)
    assert counters["n_normalized"] > 0 and counters["max_shift"] > 0 and c.n_enclosed > 0
    assert any(r["normalized"] and r["ps"] is not None for r in want) and any(r["normalized"] and r["collapsed"] for r in want)
    # parents and levels are the nested call's own
    plain = hip.call(setup[0], ["sample0#1"], flags=H.T_NESTED)
    key = lambda x: sorted(zip(x.query.tolist(), x.first.tolist(), x.level.tolist(), x.parent_query.tolist()))  # noqa: E731
    assert key(c) == key(plain)


def test_inversion_records_pass_unchanged(hip):
    g, seqs = W.tandem_indels(40, 5)
    p = W.inverted_haplotypes(W.tandem_haplotypes(40, 5, 6), 6, 3, 9, seed=4, keep=(0,))
    setup = _setup(hip, g, seqs, p)
    c, want, counters = _check(hip, setup, ["hap0"], tflags=H.T_INVERSIONS)
    raw = hip.call(setup[0], ["hap0"], flags=H.T_INVERSIONS)
    subr = lambda x: [ln for ln in x.vcf_text(date=DATE).splitlines() if "VARTYPE=SUBR" in ln]  # noqa: E731
    assert c.n_inv_records > 0 and subr(c) == subr(raw) and counters["n_normalized"] > 0
    assert all(int(c.norm_block[i]) == NIL and c.raw_pos[i] == c.pos[i] for i in range(c.n_records) if c.flags[i] & H.CALL_SUBR)


def test_every_family_of_blocks_in_one_call(hip):
    # the spacer input above at 6 units, one more haplotype that walks units 2 .. 4 of haplotype 0 backwards (the inversion
    # records), and a second reference: a reference that is not the first path of its class gets its REF spelled on its own.
    # On the restatement alone (units 6, seed 1): 35 records, of them 5 SUBR, 4 with a REF of their own, 20 normalised, 10 unchanged
    units, depth = 6, 1
    g = W.skip_nested(units, depth, seed=1)
    base = W.skip_haplotypes(units, depth, 8, seed=1)
    size = len(W._skip_template(depth, 2)[0])
    st = base.steps(0)
    a = next(k for k, (i, _) in enumerate(st) if i > 2 * size)
    b = next(k for k, (i, _) in enumerate(st) if i > 5 * size)
    back = st[:a] + [(i, 1 - r) for i, r in reversed(st[a:b])] + st[b:]
    pieces = [base.steps(k) for k in range(len(base))] + [back]
    p = W.pansn(W._paths(base.names + ["back"], [([i for i, _ in s], [r for _, r in s]) for s in pieces]), samples=5)
    _, snp, _, _, _ = W._skip_template(depth, 2)
    seqs = ["A" if s[0] < 0 else "CG"[s[1]] for s in snp] * units
    setup = _setup(hip, g, seqs, p)
    flags = H.T_NESTED | H.T_INVERSIONS
    c, want, counters = _check(hip, setup, ["sample0#1", "sample1#2"], tflags=flags)
    flubble = [r for r in want if r["vartype"] != "SUBR"]
    assert len(flubble) < len(want)                         # an inversion block
    assert any(not r["ref_is_rep"] for r in flubble)        # an extra block
    assert any(r["normalized"] for r in flubble)            # a normalised block
    assert any(not r["normalized"] for r in flubble)        # a record that only has its class block
    c2, _, _ = _check(hip, setup, ["sample0#1", "sample1#2"], tflags=flags | H.T_FORCE_TIER2)
    assert c2.vcf_text(date=DATE) == c.vcf_text(date=DATE)


# ---- unchanged
def test_vcfwave_graph_and_calls_without_the_profile(hip, golden_dir):
    setup = _fixture_setup(hip, golden_dir, VCFWAVE)
    f, sites, names, steps, sq = setup
    c, want, counters = _check(hip, setup, ["HG1"])
    assert counters["n_normalized"] == 0 and (want[0]["ref"], want[0]["alts"]) == ("CGT", ["TGA", "CGTACGTACGTA"])
    raw = hip.call(f, ["HG1"])
    body = lambda t: [ln for ln in t.splitlines() if not ln.startswith("##")]  # noqa: E731
    assert body(c.vcf_text(date=DATE)) == body(raw.vcf_text(date=DATE))
    assert raw.vcf_text(date=DATE) == V.vcf_text(names, steps, sq, V.call(sites, names, steps, sq, ["HG1"]), ["HG1"], date=DATE)
    # without the profile nothing moves and the new fields say so
    g, seqs = W.tandem_indels(60, 7)
    setup = _setup(hip, g, seqs, W.tandem_haplotypes(60, 7, 6))
    f, sites, names, steps, sq = setup
    vraw = V.call(sites, names, steps, sq, ["hap0"])
    for kw in (dict(), dict(profile="raw-graph"), dict(flags=H.T_FORCE_TIER2)):
        raw = hip.call(f, ["hap0"], **kw)
        assert raw.vcf_text(date=DATE) == V.vcf_text(names, steps, sq, vraw, ["hap0"], date=DATE)
        assert raw.raw_pos.tolist() == raw.pos.tolist() == [r["pos"] for r in vraw] and set(raw.norm_block.tolist()) == {NIL}
        assert not raw.norm_shift.any() and not raw.norm_chop.any() and not raw.norm_trim.any() and not (raw.flags & H.CALL_NORMALIZED).any()
        assert (raw.n_normalized, raw.max_shift, raw.n_norm_compared) == (0, 0, 0)
    nraw = hip.call(f, ["hap0"], flags=H.T_NESTED)
    assert nraw.vcf_text(date=DATE) == N.vcf_text(names, steps, sq, N.call(sites, names, steps, sq, ["hap0"]), ["hap0"], date=DATE)


# ---- differential.  Seeds 1, 2 and 3: the restatement alone gives 195, 192 and 192 changed records of 200 sites and a
# largest shift of 239, 233 and 242 bases (repeats of up to 40 copies of up to 6 bases)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tandem_indels(hip, seed):
    g, seqs = W.tandem_indels(200, seed)
    setup = _setup(hip, g, seqs, W.tandem_haplotypes(200, seed, 6))
    c, want, counters = _check(hip, setup, ["hap0"])
    assert counters["n_normalized"] > 0 and counters["max_shift"] >= 64
    if seed == 1:
        _check(hip, setup, ["hap0", "hap3"], tflags=H.T_FORCE_TIER2)


# ---- more samples than lanes
@pytest.mark.parametrize("ref", CC.REFS)
def test_wide_cohort(hip, ref):
    """131 samples, 261 slots (tests/cohort_cases.py) under the profile: the records' counts and genotypes ride along unchanged."""
    g, p = CC.wide_chain()
    setup = _setup(hip, g, CC.wide_sequences(g), p)
    c, want, counters = _check(hip, setup, [ref])
    assert c.n_slots == 261 and len(want) == 12
    assert c.gt.tolist() == [[H.GT_MISSING if v is None else v for v in r["slots"]] for r in want]
    _check(hip, setup, [ref], tflags=H.T_FORCE_TIER2 | H.T_INVERSIONS)

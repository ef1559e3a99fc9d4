"""What the VCF comparison and the haplotype comparison share (vcf_pair.hpp: the host builder, the items, the two tiers over a
policy, the hand-off in one block): the two calls agree on one hand-written pair wherever they run the same code, on both sides
of the tier threshold and of a ballot's 64 bytes; and calls that alternate on one context, on pairs of different sizes, see
nothing of each other's workspace or results."""
import numpy as np
import pytest

import vcfhap_cases as K
from povu_amd import HipDecomposer
from povu_amd import hip as H

pytestmark = pytest.mark.gpu
KC = K.K  # vcfcmp_cases
LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 130)  # of the shorter of REF and ALT: both sides of TIER1_BYTES and of a ballot, three ballots
SHARED = ("item_record_a", "item_record_b", "item_alt_a", "item_alt_b", "n_items_a", "n_items_b", "sample_col_a", "sample_col_b", "n_common_samples")


def pair_rows(chrom="c"):
    """One CHROM, plain REFs that do not touch.  Per length: REF == ALT but for case (trims fully), a first byte that differs, a
    last byte that differs, a symbolic ALT, an ALT with a `]` behind byte 64."""
    rng = np.random.default_rng(11)
    rows, pos = [], 10
    for n in LENGTHS:
        ref = K.bases(rng, n)
        alts = (ref.lower(), K.other(ref[0]) + ref[1:], ref[:-1] + K.other(ref[-1]), "<DEL>", K.bases(rng, 70) + "]" + chrom + ":5]")
        for k, alt in enumerate(alts):
            rows.append((chrom, pos, f"n{n}k{k}", ref, alt, ["1|0", "0|1"] if k % 2 else ["0|1", "1|1"]))
            pos += 300
    return rows


def pair_p():
    rows = pair_rows()
    flipped = [(c, p, i, r, a.swapcase() if not a.startswith("<") else a, g[::-1]) for c, p, i, r, a, g in rows[::2]]
    return K.vcf(["s1", "x"], rows), K.vcf(["y", "s1"], flipped + rows[1::4]), rows


@pytest.fixture(scope="module")
def hip():
    """A context that never sees a graph."""
    d = HipDecomposer(0)
    yield d
    d.close()


def test_the_two_calls_agree_where_they_share_code(hip):
    a, b, rows = pair_p()
    rows_b = [ln.split("\t") for ln in b.splitlines()[2:]]
    texts = {"a": [(r[3], r[4]) for r in rows], "b": [(f[3], f[4]) for f in rows_b]}
    n_long = sum(min(len(r), len(t)) > 32 for side in "ab" for r, t in texts[side])
    results = {}
    for force in (False, True):
        c, h = hip.compare_vcfs(a, b, force_tier2=force), hip.compare_haplotypes(a, b, force_tier2=force)
        results[force] = (c, h)
        have_c, have_h = KC.lib_arrays(c), K.lib_arrays(h)
        for k in SHARED:
            assert have_c[k] == have_h[k], (k, force)
        assert c.n_common_samples == 1 and c.sample_col_a.tolist() == [0] and c.sample_col_b.tolist() == [1]
        assert c.n_items_a == len(rows) and c.n_items_b == len(rows_b)
        n_all = c.n_items_a + c.n_items_b
        assert c.n_tier2 == h.n_tier2 == (n_all if force else n_long) and 0 < n_long < n_all
        for side in "ab":
            m_state, h_state = getattr(c, f"item_state_{side}"), getattr(h, f"item_state_{side}")
            assert ((m_state == H.M_SKIPPED) == (h_state == H.H_UNSPELLED)).all() and (h_state != H.H_UNPLACED).all()
            rec, alt = getattr(c, f"item_record_{side}").tolist(), getattr(c, f"item_alt_{side}").tolist()
            assert alt == [1] * len(alt)
            m_suffix, h_suffix = getattr(c, f"item_suffix_{side}").tolist(), getattr(h, f"item_suffix_{side}").tolist()
            n_keyed = 0
            for i, r in enumerate(rec):
                if m_state[i] == H.M_SKIPPED:
                    continue
                ref, text = texts[side][r]
                # vm_trim_limit = vh_trim_limit - 1 over one byte predicate
                assert m_suffix[i] == min(h_suffix[i], min(len(ref), len(text)) - 1), (side, i, force)
                n_keyed += 1
            assert side == "b" or n_keyed == 3 * len(LENGTHS)  # (of five cases a length, a symbolic ALT and a breakend are skipped)
    assert KC.digest(results[False][0]) == KC.digest(results[True][0])  # equal but for n_tier2
    assert K.digest(results[False][1]) == K.digest(results[True][1])


def _fresh(call, a, b):
    d = HipDecomposer(0)
    try:
        return (KC.digest(d.compare_vcfs(a, b)) if call == "compare" else K.digest(d.compare_haplotypes(a, b)))
    finally:
        d.close()


def test_alternating_calls_in_one_context_see_no_stale_workspace():
    """compare(P), haplotypes(Q), compare(P), haplotypes(P), compare(Q) on one context, every result against the same call on a
    fresh context.  Once with Q a golden pair (the largest: every golden pair is smaller than P) and once with Q the rows of P
    on three CHROMs, which has more records, items and tasks than P: the arenas are carved anew both ways."""
    a, b, rows = pair_p()
    P = (a, b)
    fx = "vcfwave-complex-decomposition"
    golden_q = (K.golden(fx, "raw_graph"), K.golden(fx, "decomposed"))
    big_rows = [row for chrom in "cde" for row in pair_rows(chrom)]
    big_q = (K.vcf(["s1", "x", "z"], [r[:5] + (r[5] + ["1|1"],) for r in big_rows]), K.vcf(["z", "s1"], big_rows[1::2]))
    assert len(big_rows) == 3 * len(rows)
    want = {(call, name): _fresh(call, *pair) for call in ("compare", "haplotypes") for name, pair in (("P", P),)}
    for Q in (golden_q, big_q):
        want.update({(call, "Q"): _fresh(call, *Q) for call in ("compare", "haplotypes")})
        d = HipDecomposer(0)
        try:
            held = d.compare_vcfs(*P)
            assert KC.digest(held) == want["compare", "P"]
            assert K.digest(d.compare_haplotypes(*Q)) == want["haplotypes", "Q"]
            assert KC.digest(d.compare_vcfs(*P)) == want["compare", "P"]
            assert K.digest(d.compare_haplotypes(*P)) == want["haplotypes", "P"]
            assert KC.digest(d.compare_vcfs(*Q)) == want["compare", "Q"]
            assert KC.digest(held) == want["compare", "P"]  # the first result's block was not written again
        finally:
            d.close()

"""Deterministic synthetic bidirected graphs for parity tests and bench.py.

The shapes are the ones SURVEY.md section 8(d) fixes for BASELINE.json's
configs.  A graph is returned as a :class:`Links` record: segment ids in
ascending order plus one row per GFA L-line, already translated to vertex
*indices* and sides the way the loader does (`+` on the source = right side,
`+` on the sink = left side; reference src/mto/from_gfa.cpp:223-243).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

L, R = 0, 1


@dataclass
class Links:
    vid: np.ndarray  # uint32 [V] ascending segment ids
    v1: np.ndarray   # uint32 [E] vertex idx
    s1: np.ndarray   # uint8  [E] side (0 = l, 1 = r)
    v2: np.ndarray   # uint32 [E]
    s2: np.ndarray   # uint8  [E]

    @property
    def n_vtx(self) -> int:
        return int(self.vid.shape[0])

    @property
    def n_links(self) -> int:
        return int(self.v1.shape[0])

    def to_gfa(self, seqs=None) -> str:
        """GFA text: S lines first (sequence `A`, or seqs[k] for vertex k when given), then L lines, all `0M`."""
        out = ["H\tVN:Z:1.0"]
        if seqs is None:
            out += [f"S\t{i}\tA" for i in self.vid.tolist()]
        else:
            out += [f"S\t{i}\t{q}" for i, q in zip(self.vid.tolist(), seqs)]
        vid = self.vid
        for a, sa, b, sb in zip(self.v1.tolist(), self.s1.tolist(), self.v2.tolist(), self.s2.tolist()):
            out.append(f"L\t{vid[a]}\t{'+' if sa == R else '-'}\t{vid[b]}\t{'+' if sb == L else '-'}\t0M")
        return "\n".join(out) + "\n"


def _mk(vid, v1, s1, v2, s2) -> Links:
    return Links(np.ascontiguousarray(vid, dtype=np.uint32), np.ascontiguousarray(v1, dtype=np.uint32),
                 np.ascontiguousarray(s1, dtype=np.uint8), np.ascontiguousarray(v2, dtype=np.uint32),
                 np.ascontiguousarray(s2, dtype=np.uint8))


def from_plus_links(vid, src_idx, dst_idx) -> Links:
    """All links `a + b +`."""
    e = len(src_idx)
    return _mk(vid, src_idx, np.full(e, R), dst_idx, np.full(e, L))


def chain_of_bubbles(k: int) -> Links:
    """BASELINE config 2: K units, ids 1..3K+1; unit i has a=3i+1, x=a+1,
    y=a+2, b=a+3 and links a>x a>y x>y x>b y>b a>b.  K=333333 -> 1 000 000 segments,
    1 999 998 links, one component, K flubbles."""
    vid = np.arange(1, 3 * k + 2, dtype=np.uint32)
    a = 3 * np.arange(k, dtype=np.int64)  # vertex idx of `a`
    src = np.stack([a, a, a + 1, a + 1, a + 2, a], axis=1).reshape(-1)
    dst = np.stack([a + 1, a + 2, a + 2, a + 3, a + 3, a + 3], axis=1).reshape(-1)
    return from_plus_links(vid, src, dst)


def nested_towers(depth: int, towers: int) -> Links:
    """BASELINE config 5 shape: per tower a_0..a_{d-1}, c, b_{d-1}..b_0 (ids in
    that order), links a_i>a_{i+1} and b_{i+1}>b_i interleaved, a_{d-1}>c, c>b_{d-1}, bypasses
    a_i>b_i, towers chained b_0(t)>a_0(t+1)."""
    d = depth
    per = 2 * d + 1
    vid = np.arange(1, per * towers + 1, dtype=np.uint32)
    src, dst = [], []
    i = np.arange(d - 1, dtype=np.int64)
    a = lambda j: j            # noqa: E731  idx inside tower
    b = lambda j: 2 * d - j    # noqa: E731  b_j : b_{d-1} = d+1 ... b_0 = 2d
    c = d
    inter_s = np.stack([a(i), b(i + 1)], axis=1).reshape(-1)
    inter_d = np.stack([a(i + 1), b(i)], axis=1).reshape(-1)
    j = np.arange(d, dtype=np.int64)
    ts = np.concatenate([inter_s, [a(d - 1), c], a(j)])
    td = np.concatenate([inter_d, [c, b(d - 1)], b(j)])
    for t in range(towers):
        base = t * per
        src.append(ts + base)
        dst.append(td + base)
        if t + 1 < towers:
            src.append(np.array([b(0) + base]))
            dst.append(np.array([a(0) + base + per]))
    return from_plus_links(vid, np.concatenate(src), np.concatenate(dst))


class _PCG32:
    """PCG32 (XSH-RR) so the HPRC-shaped generator is reproducible everywhere."""

    def __init__(self, seed: int, seq: int = 54):
        self.m = (1 << 64) - 1
        self.state = 0
        self.inc = ((seq << 1) | 1) & self.m
        self.next()
        self.state = (self.state + seed) & self.m
        self.next()

    def next(self) -> int:
        old = self.state
        self.state = (old * 6364136223846793005 + self.inc) & self.m
        xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((xs >> rot) | (xs << ((-rot) & 31))) & 0xFFFFFFFF


def hprc_shaped(backbone_sizes, seed: int = 20260612, tiny: int = 0) -> Links:
    """HPRC-shaped multi-component graph: per component a backbone of
    N segments with bubble density 0.35/segment; bubble mix SNP 70 % / indel 20 % / nested 8 % /
    inversion 2 %; plus `tiny` small (<50 segment) components.  Uses numpy's PCG64 for the bulk
    draws (seeded) -- the graph is deterministic for a given numpy version and is always fed
    to both the oracle and the HIP path in the same process."""
    rng = np.random.Generator(np.random.PCG64(seed))
    vids, s_all, d_all, s1_all, s2_all = [], [], [], [], []
    next_id = 1
    base_idx = 0

    def emit_component(n_backbone: int):
        nonlocal next_id, base_idx
        kinds = rng.random(n_backbone - 1)
        has = rng.random(n_backbone - 1) < 0.35
        # extra segments per backbone gap: SNP 2 (two alleles), indel 1, nested 4, inversion 0
        k_snp = has & (kinds < 0.70)
        k_indel = has & (kinds >= 0.70) & (kinds < 0.90)
        k_nest = has & (kinds >= 0.90) & (kinds < 0.98)
        k_inv = has & (kinds >= 0.98)
        extra = np.zeros(n_backbone - 1, dtype=np.int64)
        extra[k_snp] = 2
        extra[k_indel] = 1
        extra[k_nest] = 4
        # layout: backbone segment i followed by its gap's extra segments
        stride = np.concatenate([[0], np.cumsum(1 + extra)])
        bb = stride[:-1] if len(stride) == n_backbone else stride[:n_backbone]
        bb = np.concatenate([bb, [stride[-1]]])[:n_backbone]
        n_local = int(stride[-1] + 1)
        a = bb[:-1]
        b = bb[1:]
        S, D, S1, S2 = [], [], [], []

        def plus(s, d):
            S.append(s)
            D.append(d)
            S1.append(np.full(len(s), R, dtype=np.uint8))
            S2.append(np.full(len(s), L, dtype=np.uint8))

        plain = ~has
        plus(a[plain], b[plain])
        # SNP: a>x a>y x>b y>b
        m = k_snp
        x, y = a[m] + 1, a[m] + 2
        plus(a[m], x); plus(a[m], y); plus(x, b[m]); plus(y, b[m])
        # indel: a>x x>b a>b
        m = k_indel
        x = a[m] + 1
        plus(a[m], x); plus(x, b[m]); plus(a[m], b[m])
        # nested: a>p p>q p>r q>s r>s s>b a>b   (p..s = a+1..a+4)
        m = k_nest
        p_, q_, r_, s_ = a[m] + 1, a[m] + 2, a[m] + 3, a[m] + 4
        plus(a[m], p_); plus(p_, q_); plus(p_, r_); plus(q_, s_); plus(r_, s_); plus(s_, b[m]); plus(a[m], b[m])
        # inversion: a>b plus the reverse link `b - a -` written as a `+ -` style link a+ -> b-
        m = k_inv
        plus(a[m], b[m])
        S.append(a[m]); D.append(b[m])
        S1.append(np.full(int(m.sum()), R, dtype=np.uint8)); S2.append(np.full(int(m.sum()), R, dtype=np.uint8))
        s = np.concatenate(S); d = np.concatenate(D)
        s1 = np.concatenate(S1); s2 = np.concatenate(S2)
        # L-line order: by source backbone position then as emitted (stable)
        order = np.argsort(np.minimum(s, d), kind="stable")
        vids.append(np.arange(next_id, next_id + n_local, dtype=np.uint32))
        s_all.append(s[order] + base_idx); d_all.append(d[order] + base_idx)
        s1_all.append(s1[order]); s2_all.append(s2[order])
        next_id += n_local
        base_idx += n_local

    for n in backbone_sizes:
        emit_component(int(n))
    for _ in range(tiny):
        emit_component(int(rng.integers(3, 20)))
    return _mk(np.concatenate(vids), np.concatenate(s_all), np.concatenate(s1_all), np.concatenate(d_all),
               np.concatenate(s2_all))


def hprc_circular(n_backbone: int, seed: int = 20260612) -> Links:
    """One HPRC-shaped component closed into a ring (the last backbone segment links back to the first): no side is left
    without a link, so the component has NO tip -- from_bd starts at (l, vertex 0) without a dummy root and gives that root a
    back edge to itself (spanning_tree.cpp:433-438).  The shape of a circular chromosome / plasmid / mitochondrial genome."""
    g = hprc_shaped([n_backbone], seed=seed)
    last = g.n_vtx - 1
    return _mk(g.vid, np.concatenate([g.v1, [last]]), np.concatenate([g.s1, np.array([R], dtype=np.uint8)]),
               np.concatenate([g.v2, [0]]), np.concatenate([g.s2, np.array([L], dtype=np.uint8)]))


def hub_on_chain(k_units: int = 100000, hub_links: int = 200000, seed: int = 1) -> Links:
    """A chain of bubbles with ONE hub segment: `hub_links` links from the r side of segment 0 to the l sides of segments drawn
    uniformly from the chain (repeats included): one side with 2 * 10^5 links, one 2-edge-connected class that holds most of
    the graph.  Nothing like a pangenome; the shape that finds quadratic corners."""
    base = chain_of_bubbles(k_units)
    rng = np.random.default_rng(seed)
    hv2 = rng.integers(1, base.n_vtx, size=hub_links)
    return _mk(base.vid, np.concatenate([base.v1, np.zeros(hub_links, dtype=np.int64)]),
               np.concatenate([base.s1, np.full(hub_links, R, dtype=np.uint8)]), np.concatenate([base.v2, hv2]),
               np.concatenate([base.s2, np.full(hub_links, L, dtype=np.uint8)]))


# chr1..22, X, Y lengths in Mbp: the relative sizes of the 24 large components of a whole-genome pangenome
CHR_MBP = (248, 242, 198, 190, 182, 171, 159, 145, 138, 134, 135, 133, 114, 107, 102, 90, 83, 80, 59, 64, 47, 51, 156, 57)


def hprc_whole_genome(total_segments: float = 1e8, tiny: int = 2000, seed: int = 20260612) -> Links:
    """BASELINE config 4: 24 HPRC-shaped components with sizes proportional to chr1..22,X,Y
    summing to ~`total_segments` segments, plus `tiny` components of < 50 segments.  At the default size:
    99 860 187 segments / 122 435 438 links / 2 024 components."""
    # the generator emits ~1.675 segments per backbone segment
    sizes = [max(8, int(total_segments / 1.675 * m / sum(CHR_MBP))) for m in CHR_MBP]
    return hprc_shaped(sizes, seed=seed, tiny=tiny)


def hprc_tangled(n_backbone: int, seed: int = 20260612, tangle_every: int = 20000, max_tangle: int = 200000,
                 shuffle_links: bool = True) -> Links:
    """HPRC-shaped component with TANGLES: the chain of small bubbles of `hprc_shaped`, and every ~`tangle_every`
    backbone segments a tangle replaces a bubble -- `n` extra segments (heavy-tailed: n = 100 * 10^(3u), u uniform,
    capped at `max_tangle`, i.e. 10^2 .. 10^5+ segments) wired by a random spanning path plus 0.6 n random links with
    random sides (inversions, self loops, parallel links), entered from the backbone segment before it and left to the
    one behind it.  Each tangle is one large 2-edge-connected class (the case a chain of bubbles never produces); with
    `shuffle_links` the L lines of a tangle come in random order instead of sorted along the backbone."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = hprc_shaped([n_backbone], seed=seed)
    nv = base.n_vtx
    # backbone vertices of `base`: recover them as the articulation-free spine is not needed -- tangles hang between
    # two consecutive vertex indices chosen at random positions (a link a -> b of the spine is rerouted through the tangle)
    v1, v2, s1, s2 = [base.v1.astype(np.int64)], [base.v2.astype(np.int64)], [base.s1], [base.s2]
    n_t = max(1, n_backbone // tangle_every)
    # candidate attachment links: plain backbone links (+ +) between consecutive vertices
    plain = np.flatnonzero((base.v2.astype(np.int64) - base.v1.astype(np.int64) == 1) & (base.s1 == R) & (base.s2 == L))
    pick = np.sort(rng.choice(plain, size=min(n_t, len(plain)), replace=False))
    keep = np.ones(base.n_links, dtype=bool)
    keep[pick] = False
    nxt = nv
    ex_v1, ex_v2, ex_s1, ex_s2 = [], [], [], []
    for e in pick.tolist():
        n = int(min(max_tangle, 100 * 10 ** (3 * rng.random())))
        a, b = int(base.v1[e]), int(base.v2[e])
        ids = np.arange(nxt, nxt + n, dtype=np.int64)
        nxt += n
        perm = rng.permutation(ids)
        # spanning path through the tangle, entered from a and left to b
        p1 = np.concatenate([[a], perm])
        p2 = np.concatenate([perm, [b]])
        m = int(0.6 * n)
        r1 = rng.choice(ids, size=m)
        r2 = rng.choice(ids, size=m)
        t1 = np.concatenate([p1, r1]); t2 = np.concatenate([p2, r2])
        ts1 = np.concatenate([np.full(len(p1), R), rng.integers(0, 2, size=m)]).astype(np.uint8)
        ts2 = np.concatenate([np.full(len(p2), L), rng.integers(0, 2, size=m)]).astype(np.uint8)
        if shuffle_links:
            o = rng.permutation(len(t1))
            t1, t2, ts1, ts2 = t1[o], t2[o], ts1[o], ts2[o]
        ex_v1.append(t1); ex_v2.append(t2); ex_s1.append(ts1); ex_s2.append(ts2)
    n_all = nxt
    vid = np.arange(1, n_all + 1, dtype=np.uint32)
    V1 = np.concatenate([base.v1.astype(np.int64)[keep]] + ex_v1)
    V2 = np.concatenate([base.v2.astype(np.int64)[keep]] + ex_v2)
    S1 = np.concatenate([base.s1[keep]] + ex_s1)
    S2 = np.concatenate([base.s2[keep]] + ex_s2)
    return _mk(vid, V1, S1, V2, S2)


def random_bidirected(n_vtx: int, n_links: int, seed: int, self_loops: bool = True,
                      connected: bool = False) -> Links:
    """Differential-fuzz input: random sides, parallel links, self loops, several components."""
    rng = np.random.Generator(np.random.PCG64(seed))
    vid = np.sort(rng.choice(np.arange(1, 4 * n_vtx + 1), size=n_vtx, replace=False)).astype(np.uint32)
    v1 = rng.integers(0, n_vtx, size=n_links)
    v2 = rng.integers(0, n_vtx, size=n_links)
    if connected and n_vtx > 1:
        k = min(n_links, n_vtx - 1)
        v1[:k] = np.arange(k)
        v2[:k] = np.arange(1, k + 1)
    if not self_loops:
        same = v1 == v2
        v2[same] = (v2[same] + 1) % n_vtx
    s1 = rng.integers(0, 2, size=n_links)
    s2 = rng.integers(0, 2, size=n_links)
    # mostly "forward" links so that long chains / bubbles appear
    fwd = rng.random(n_links) < 0.7
    s1[fwd] = R
    s2[fwd] = L
    return _mk(vid, v1, s1, v2, s2)


def bubble_zoo(n_comp: int, sites: int, seed: int, shuffle_ids: bool = True) -> Links:
    """Many small components, each a backbone whose sites are small motifs drawn at random: SNPs, multi-allelic sites,
    indels, the chain-of-bubbles unit, repeated links, inversions, self loops (both kinds), a bubble nested in an allele,
    small random tangles, dangling hairpins, flipped interior segments.  The leaf flubbles of such graphs come in every
    shape the two relabelling passes of `-s` (find_tiny / find_parallel) distinguish, and the components are small enough
    that a back-edge INDEX often equals a tree vertex index (tiny.cpp:52-56 compares the two)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    links = []  # (a, side_a, b, side_b) over provisional vertex numbers
    nv = 0

    def new():
        nonlocal nv
        nv += 1
        return nv - 1

    def fwd(a, b, fa=False, fb=False):  # a -> b; a flipped segment presents its other side
        links.append((a, L if fa else R, b, R if fb else L))

    for _ in range(n_comp):
        prev = new()
        anchors = []
        for _ in range(int(rng.integers(1, sites + 1))):
            nxt = new()
            m = int(rng.integers(0, 16))
            flip = bool(rng.random() < 0.25)
            if m == 0:  # SNP
                for _ in range(2):
                    x = new()
                    fwd(prev, x, fb=flip)
                    fwd(x, nxt, fa=flip)
            elif m == 1:  # multi-allelic
                for _ in range(int(rng.integers(3, 7))):
                    x = new()
                    fwd(prev, x)
                    fwd(x, nxt)
            elif m == 2:  # indel
                x = new()
                fwd(prev, x, fb=flip)
                fwd(x, nxt, fa=flip)
                fwd(prev, nxt)
            elif m == 3:  # the unit of chain_of_bubbles
                x, y = new(), new()
                fwd(prev, x), fwd(prev, y), fwd(x, y), fwd(x, nxt), fwd(y, nxt), fwd(prev, nxt)
            elif m == 4:  # repeated links
                x = new()
                for _ in range(int(rng.integers(2, 4))):
                    fwd(prev, x)
                fwd(x, nxt)
                if rng.random() < 0.5:
                    fwd(x, nxt)
            elif m == 5:  # inversion: the allele is entered from both ends
                x = new()
                fwd(prev, x), fwd(x, nxt)
                fwd(prev, x, fb=True), fwd(x, nxt, fa=True)
            elif m == 6:  # self loops
                x = new()
                fwd(prev, x), fwd(x, nxt)
                if rng.random() < 0.5:
                    links.append((x, R, x, L))
                else:
                    s = int(rng.integers(0, 2))
                    links.append((x, s, x, s))
                if rng.random() < 0.5:
                    fwd(prev, nxt)
            elif m == 7:  # a SNP nested in one allele
                x, y, a, b = new(), new(), new(), new()
                fwd(prev, x), fwd(x, a), fwd(x, b), fwd(a, y), fwd(b, y), fwd(y, nxt)
                z = new()
                fwd(prev, z), fwd(z, nxt)
            elif m == 8:  # small random tangle between the anchors
                k = int(rng.integers(2, 6))
                xs = [new() for _ in range(k)]
                fwd(prev, xs[0]), fwd(xs[-1], nxt)
                for _ in range(int(rng.integers(k, 3 * k))):
                    a, b = int(rng.integers(0, k)), int(rng.integers(0, k))
                    links.append((xs[a], int(rng.integers(0, 2)), xs[b], int(rng.integers(0, 2))))
                for i in range(k - 1):
                    fwd(xs[i], xs[i + 1])
            elif m == 9:  # dangling hairpin and a plain step
                x = new()
                fwd(prev, x)
                links.append((x, R, x, R))
                fwd(prev, nxt)
            elif m == 10:  # two alleles of different length
                x, y, z = new(), new(), new()
                fwd(prev, x), fwd(x, nxt), fwd(prev, y), fwd(y, z), fwd(z, nxt)
            elif m == 11:  # funnel: several alleles merge into one segment before the site ends; plus the direct step
                k = int(rng.integers(3, 6))
                x = new()
                for _ in range(k):
                    y = new()
                    fwd(prev, y), fwd(y, x)
                fwd(x, nxt), fwd(prev, nxt)
            elif m == 12:  # the funnel the other way round
                k = int(rng.integers(3, 6))
                x = new()
                fwd(prev, x)
                for _ in range(k):
                    y = new()
                    fwd(x, y), fwd(y, nxt)
                fwd(prev, nxt)
            elif m == 13:  # a segment hanging off the site, reached from earlier anchors as well
                x = new()
                fwd(prev, x)
                fwd(prev, nxt)
                for a in anchors[-3:]:
                    if rng.random() < 0.6:
                        fwd(a, x)
                if rng.random() < 0.5 and anchors:
                    fwd(x, anchors[int(rng.integers(0, len(anchors)))], fb=True)
            elif m == 14:  # a tip hanging off the far end of the site
                x = new()
                fwd(prev, nxt)
                links.append((nxt, L, x, int(rng.integers(0, 2))))
            else:  # plain step, sometimes doubled
                fwd(prev, nxt)
                if rng.random() < 0.3:
                    fwd(prev, nxt)
            anchors.append(prev)
            prev = nxt
    perm = rng.permutation(nv) if shuffle_ids else np.arange(nv)
    arr = np.array(links, dtype=np.int64).reshape(-1, 4)
    order = rng.permutation(len(arr)) if shuffle_ids else np.arange(len(arr))
    arr = arr[order]
    vid = np.arange(1, nv + 1, dtype=np.uint32)
    return _mk(vid, perm[arr[:, 0]], arr[:, 1], perm[arr[:, 2]], arr[:, 3])


def hanger_family(prefix: int, suffix: int, variant: int, direct_first: bool = True) -> Links:
    """One component: `prefix` plain steps, an indel site (prev -> y -> nxt and prev -> nxt) with one more segment x
    hanging off the inner side of nxt, then `suffix` plain steps.  variant 0: x carries a loop between its two sides
    (its tree edge is a bridge: x gets a simplifying back edge); variant 1: x's far side is a tip and its near side is also
    reached from the first segment of the component (an ordinary back edge out of x); variant 2: both.  As the prefix
    grows, the tree vertex idx of the site's boundary sweeps across the back-edge indices of x's edges -- the
    coincidence tiny.cpp:52-56 turns into a 'tiny' label."""
    links = []
    n = prefix + 4 + suffix + 1
    first = 0
    for i in range(prefix):
        links.append((i, R, i + 1, L))
    prev, y, nxt, x = prefix, prefix + 1, prefix + 2, prefix + 3
    site = [(prev, R, nxt, L), (prev, R, y, L), (y, R, nxt, L)]
    if not direct_first:
        site = site[1:] + site[:1]
    links += site
    links.append((nxt, L, x, L))
    if variant in (0, 2):
        links.append((x, R, x, L))
    if variant in (1, 2) and prefix > 0:
        links.append((first, R, x, L))
    last = nxt
    for i in range(suffix):
        links.append((last, R, prefix + 4 + i, L))
        last = prefix + 4 + i
    arr = np.array(links, dtype=np.int64)
    return _mk(np.arange(1, n + 1, dtype=np.uint32), arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3])


# ---- paths (haplotypes) over a graph: the input of HipDecomposer.traversals


@dataclass
class Paths:
    names: list      # [n] path names (GFA P-line order)
    off: np.ndarray  # uint64 [n + 1] steps of path k: [off[k], off[k + 1])
    ids: np.ndarray  # uint32 [off[-1]] segment id of every step
    rev: np.ndarray  # uint8  [off[-1]] 0 '>' (GFA '+'), 1 '<' (GFA '-')

    def __len__(self) -> int:
        return len(self.names)

    @property
    def n_steps(self) -> int:
        return int(self.off[-1])

    def steps(self, k: int):
        """[(segment id, 0 | 1), ...] of path k."""
        a, b = int(self.off[k]), int(self.off[k + 1])
        return list(zip(self.ids[a:b].tolist(), self.rev[a:b].tolist()))

    def to_gfa(self) -> str:
        """P lines, one per path (append to Links.to_gfa() for one GFA)."""
        out = []
        for k, name in enumerate(self.names):
            a, b = int(self.off[k]), int(self.off[k + 1])
            ids, rev = self.ids[a:b].tolist(), self.rev[a:b].tolist()
            out.append(f"P\t{name}\t" + ",".join(f"{i}{'-' if r else '+'}" for i, r in zip(ids, rev)) + "\t*")
        return "\n".join(out) + ("\n" if out else "")


def _paths(names, pieces) -> Paths:
    """Paths from per-path (ids, rev) arrays."""
    lens = np.array([len(i) for i, _ in pieces], dtype=np.uint64)
    off = np.zeros(len(pieces) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    ids = np.concatenate([np.asarray(i, dtype=np.uint32) for i, _ in pieces]) if pieces else np.zeros(0, np.uint32)
    rev = np.concatenate([np.asarray(r, dtype=np.uint8) for _, r in pieces]) if pieces else np.zeros(0, np.uint8)
    return Paths(list(names), off, ids, rev)


def _side_csr(links: Links):
    """Per side (2 vertex + side): the other ends (2 u + side) of its links, CSR."""
    nS = 2 * links.n_vtx
    a = 2 * links.v1.astype(np.int64) + links.s1
    b = 2 * links.v2.astype(np.int64) + links.s2
    src = np.concatenate([a, b])
    dst = np.concatenate([b, a])
    order = np.argsort(src, kind="stable")
    src, dst = src[order], dst[order]
    off = np.zeros(nS + 1, dtype=np.int64)
    np.add.at(off, src + 1, 1)
    return np.cumsum(off), dst


def random_walk_paths(links: Links, n: int, length: int, seed: int, jump: float = 0.0) -> Paths:
    """`n` paths of up to `length` steps that follow the links: from a random step, each next step goes out of the current
    step's exit side over a random link ('>' enters a segment by its l side and leaves by r).  A path ends early at a
    side without links.  With `jump` > 0 every next step is, with that probability, a random (segment, orientation)
    instead -- steps no link joins, which make scans meet stray boundaries (noise_paths)."""
    rng = np.random.default_rng(seed)
    off, dst = _side_csr(links)
    V = links.n_vtx
    cur = 2 * rng.integers(0, V, size=n) + rng.integers(0, 2, size=n)  # step word: 2 v + orientation (entered side)
    alive = np.ones(n, dtype=bool)
    out = np.full((n, length), -1, dtype=np.int64)
    for t in range(length):
        out[alive, t] = cur[alive]
        ex = cur ^ 1  # exit side: the other side of the segment
        deg = off[ex + 1] - off[ex]
        pick = off[ex] + (rng.random(n) * np.maximum(deg, 1)).astype(np.int64)
        nxt = dst[np.minimum(pick, len(dst) - 1)] if len(dst) else cur
        if jump > 0:
            j = rng.random(n) < jump
            nxt = np.where(j, 2 * rng.integers(0, V, size=n) + rng.integers(0, 2, size=n), nxt)
            alive &= (deg > 0) | j
        else:
            alive &= deg > 0
        cur = nxt
    pieces = []
    for k in range(n):
        w = out[k][out[k] >= 0]
        pieces.append((links.vid[w >> 1], (w & 1).astype(np.uint8)))
    return _paths([f"walk{k}" for k in range(n)], pieces)


def noise_paths(links: Links, n: int, length: int, seed: int, jump: float = 0.2) -> Paths:
    """Random-walk paths with random jumps (see random_walk_paths): they reach every way a scan can fail -- a stray
    boundary, the end of the path, more than max_steps steps."""
    p = random_walk_paths(links, n, length, seed, jump=jump)
    p.names = [f"noise{k}" for k in range(n)]
    return p


def chain_haplotypes(k: int, n: int, seed: int, reverse_every: int = 4) -> Paths:
    """`n` haplotypes of chain_of_bubbles(k), in closed form: unit i (a = 3i + 1) is crossed by x (a + 1), by y (a + 2) or
    by the a > b skip, chosen at random; every `reverse_every`-th haplotype is written reversed ('<' steps from the last
    segment to the first).  Vectorised per haplotype: 10^8 segments x 32 haplotypes in seconds."""
    rng = np.random.default_rng(seed)
    a = 3 * np.arange(k, dtype=np.int64) + 1
    pieces = []
    for h in range(n):
        c = rng.integers(0, 3, size=k, dtype=np.int8)
        two = c < 2
        ln = np.where(two, 2, 1)
        start = np.zeros(k + 1, dtype=np.int64)
        np.cumsum(ln, out=start[1:])
        ids = np.empty(int(start[-1]) + 1, dtype=np.uint32)
        ids[start[:-1]] = a
        ids[start[:-1][two] + 1] = (a[two] + 1 + c[two]).astype(np.uint32)
        ids[-1] = 3 * k + 1
        if reverse_every and h % reverse_every == reverse_every - 1:
            pieces.append((ids[::-1].copy(), np.ones(ids.size, dtype=np.uint8)))
        else:
            pieces.append((ids, np.zeros(ids.size, dtype=np.uint8)))
    return _paths([f"hap{h}" for h in range(n)], pieces)


def random_sequences(links: Links, seed: int, max_len: int = 300, empty: float = 0.1) -> list:
    """A random sequence per vertex (index order): lengths 0 to max_len (a share `empty` of them empty, half of the rest a
    single base), mostly ACGT with some lower case and IUPAC codes -- every VARTYPE and anchoring case of a call."""
    rng = np.random.default_rng(seed)
    n = links.n_vtx
    kind = rng.random(n)
    lens = np.where(kind < empty, 0, np.where(kind < (1 + empty) / 2, 1, rng.integers(1, max_len + 1, size=n)))
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTacgtNRYKMSWBDHV", np.uint8)
    pool = alphabet[rng.integers(0, alphabet.size, size=int(lens.sum()) + 1)].tobytes().decode()
    out, at = [], 0
    for ln in lens.tolist():
        out.append(pool[at:at + ln])
        at += ln
    return out


def pansn(paths: Paths, samples: int, haps: int = 2, contig: str = "chr1") -> Paths:
    """The same paths renamed `sample<k>#<hap>#<contig>`: path j is hap (j % haps) + 1 of sample j // haps (modulo
    `samples`, so that later paths become further contigs of the same slots)."""
    names = []
    for j in range(len(paths)):
        sm = (j // haps) % samples
        rnd = j // (haps * samples)
        names.append(f"sample{sm}#{j % haps + 1}#{contig}" + (f"_{rnd}" if rnd else ""))
    return Paths(names, paths.off, paths.ids, paths.rev)


def inverted_haplotypes(paths: Paths, n: int, min_len: int, max_len: int, seed: int, keep=()) -> Paths:
    """A copy of `paths` in which `n` random intervals of min_len to max_len steps (cut at the path's end), each in a random
    path whose index is not in `keep`, are replaced by their reverse complement: the steps backwards, every orientation
    flipped -- the haplotype walks that stretch of the graph the other way round, which is what an inversion call finds
    against a path that kept it (INTEGRATION.md "Inversion calls").  Intervals may overlap; a path shorter than min_len
    steps is left alone."""
    rng = np.random.default_rng(seed)
    ids, rev = paths.ids.copy(), paths.rev.copy()
    off = paths.off.astype(np.int64)
    pool = [k for k in range(len(paths)) if k not in set(keep) and off[k + 1] - off[k] >= max(min_len, 1)]
    for _ in range(n if pool else 0):
        k = pool[int(rng.integers(0, len(pool)))]
        ln = int(rng.integers(min_len, max_len + 1))
        a = int(off[k]) + int(rng.integers(0, int(off[k + 1] - off[k]) - min_len + 1))
        b = min(a + ln, int(off[k + 1]))
        ids[a:b] = ids[a:b][::-1].copy()
        rev[a:b] = 1 - rev[a:b][::-1]
    return Paths(list(paths.names), paths.off.copy(), ids, rev)


def _skip_template(depth: int, width: int):
    """One unit of skip_nested in local numbering (creation order = path order): per segment the skip decisions that remove
    it and its SNP (number, branch) or (-1, 0); the links; the number of decisions and SNPs."""
    anc, snp, links, n_dec, n_snp = [], [], [], [0], [0]

    def seg(a, s=(-1, 0)):
        anc.append(a)
        snp.append(s)
        return len(anc) - 1

    def unit(d, a):
        dec = n_dec[0]
        n_dec[0] += 1
        e = seg(a)
        inner = a + (dec,)
        prev = seg(inner)  # (a spacer: with it the PVST keeps the chain's sites beside the unit, not under it)
        links.append((e, prev))
        for _ in range(width):
            if d == 0:
                s = n_snp[0]
                n_snp[0] += 1
                first, x, y, last = seg(inner), seg(inner, (s, 0)), seg(inner, (s, 1)), seg(inner)
                links.extend([(first, x), (first, y), (x, last), (y, last)])
            else:
                first, last = unit(d - 1, inner)
            links.append((prev, first))
            prev = last
        z = seg(a)
        links.extend([(prev, z), (e, z)])
        return e, z
    unit(depth, ())
    return anc, snp, links, n_dec[0], n_snp[0]


def skip_nested(n_units: int, depth: int, seed: int = 0, width: int = 2) -> Links:
    """Nested sites that no PVST nests ("Nested calls"): a unit is an entry segment, a spacer, a chain of `width` links, an
    exit segment and a skip link from entry to exit; a link of the chain is a unit of depth - 1, at depth 0 a two-way SNP bubble
    (a, x | y, b).  `n_units` units joined end to end, ids 1.. in path order; 3 + 4 width segments a unit at depth 0,
    3 + width times the size below at every depth above.  (`seed` is unused: the shape is fixed; skip_haplotypes draws.)"""
    anc, _, links, _, _ = _skip_template(depth, width)
    size = len(anc)
    base = size * np.arange(n_units, dtype=np.int64)[:, None]
    la = np.array(links, dtype=np.int64)
    src = (base + la[:, 0][None, :]).reshape(-1)
    dst = (base + la[:, 1][None, :]).reshape(-1)
    join = size * np.arange(1, n_units, dtype=np.int64)
    return from_plus_links(np.arange(1, size * n_units + 1, dtype=np.uint32), np.concatenate([src, join - 1]),
                           np.concatenate([dst, join]))


def skip_haplotypes(n_units: int, depth: int, n: int, seed: int, width: int = 2) -> Paths:
    """`n` haplotypes of skip_nested(n_units, depth): each walks the units and takes every skip it meets with probability
    1/4, every SNP branch with probability 1/2; PanSN names, one sample a haplotype (`hap<k>#1#chr1`).  Vectorised over the
    units of a haplotype."""
    anc, snp, _, n_dec, n_snp = _skip_template(depth, width)
    size = len(anc)
    rng = np.random.default_rng(seed)
    ids = np.arange(1, size * n_units + 1, dtype=np.uint32).reshape(n_units, size)
    snp_id = np.array([s[0] for s in snp])
    snp_br = np.array([s[1] for s in snp])
    pieces = []
    for _ in range(n):
        skip = rng.random((n_units, n_dec)) < 0.25
        branch = rng.integers(0, 2, size=(n_units, max(n_snp, 1)))
        present = np.ones((n_units, size), dtype=bool)
        for k in range(size):
            for d in anc[k]:
                present[:, k] &= ~skip[:, d]
            if snp_id[k] >= 0:
                present[:, k] &= branch[:, snp_id[k]] == snp_br[k]
        w = ids[present]
        pieces.append((w, np.zeros(w.size, dtype=np.uint8)))
    return _paths([f"hap{h}#1#chr1" for h in range(n)], pieces)


_INSERTION_UNIT = 8  # entry, two segments of the reference arm, the insertion arm (open, SNP x | y, close), exit
_INSERTION_LINKS = [(0, 1), (1, 2), (2, 7), (0, 3), (3, 4), (3, 5), (4, 6), (5, 6), (6, 7)]


def insertion_units(n_units: int, seed: int = 0) -> Links:
    """Variation inside sequence a reference does not have ("Off-reference calls"): a unit is an entry segment, a reference arm
    of two segments, an insertion arm (open, a two-way SNP bubble x | y, close) and an exit segment; `n_units` units joined end
    to end, ids 1.. in path order, 8 segments a unit.  The unit's site is crossed by every haplotype, the SNP's only by those
    that carry the insertion.  (`seed` is unused: the shape is fixed; insertion_haplotypes draws.)"""
    size = _INSERTION_UNIT
    base = size * np.arange(n_units, dtype=np.int64)[:, None]
    la = np.array(_INSERTION_LINKS, dtype=np.int64)
    src = (base + la[:, 0][None, :]).reshape(-1)
    dst = (base + la[:, 1][None, :]).reshape(-1)
    join = size * np.arange(1, n_units, dtype=np.int64)
    return from_plus_links(np.arange(1, size * n_units + 1, dtype=np.uint32), np.concatenate([src, join - 1]),
                           np.concatenate([dst, join]))


def insertion_haplotypes(n_units: int, n: int, seed: int) -> Paths:
    """`n` haplotypes of insertion_units(n_units): each takes, per unit, the insertion arm with probability 1/2 and then a
    branch of its SNP with probability 1/2; haplotype 0 always takes the reference arm.  PanSN names, one sample a haplotype
    (`hap<k>#1#chr1`).  Vectorised over the units of a haplotype."""
    size = _INSERTION_UNIT
    rng = np.random.default_rng(seed)
    ids = np.arange(1, size * n_units + 1, dtype=np.uint32).reshape(n_units, size)
    pieces = []
    for h in range(n):
        ins = rng.random(n_units) < 0.5 if h else np.zeros(n_units, dtype=bool)
        y = rng.integers(0, 2, size=n_units).astype(bool)
        present = np.ones((n_units, size), dtype=bool)
        present[:, 1] = present[:, 2] = ~ins
        present[:, 3] = present[:, 6] = ins
        present[:, 4] = ins & ~y
        present[:, 5] = ins & y
        w = ids[present]
        pieces.append((w, np.zeros(w.size, dtype=np.uint8)))
    return _paths([f"hap{h}#1#chr1" for h in range(n)], pieces)


_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _tandem_plan(n_units: int, seed: int, max_copies: int, max_seg: int):
    """The units of tandem_indels: (sequence of every segment, ids 1.. in path order; per unit the steps every haplotype
    walks [(id, rev), ...] and the id of its bubble's segment, which follows them; the id of the closing segment)."""
    rng = np.random.default_rng(seed)
    seqs, units = [], []

    def seg(text, rev=0):
        seqs.append(text.encode().translate(_RC)[::-1].decode() if rev else text)
        return (len(seqs), rev)
    for _ in range(n_units):
        steps = [seg("".join("ACGT"[k] for k in rng.integers(0, 4, size=int(rng.integers(2, 9)))))]
        period = int(rng.integers(1, 7))
        motif = "".join("ACGT"[k] for k in rng.integers(0, 4, size=period))
        part = int(rng.integers(0, period))
        text = motif[period - part:] + motif * int(rng.integers(2, max_copies + 1))
        at = 0
        while at < len(text):
            ln = 1 if rng.random() < 0.5 else int(rng.integers(1, max_seg + 1))
            piece = text[at:at + ln]
            at += len(piece)
            if rng.random() < 0.1:
                piece = piece.lower()
            steps.append(seg(piece, int(at < len(text) and rng.random() < 0.25)))  # (the last one, the site's entry, stays '+')
        units.append((steps, seg(motif)[0]))
    return seqs, units, seg("".join("ACGT"[k] for k in rng.integers(0, 4, size=4)))[0]


def tandem_indels(n_units: int, seed: int, max_copies: int = 40, max_seg: int = 70):
    """Indels at the right end of tandem repeats ("Left-normalised calls"): (graph, sequence of every segment).  A unit is a
    flank of 2 to 8 random bases, a tandem repeat of period 1 to 6 with 2 to `max_copies` copies behind a partial one, cut
    into segments of random lengths (half of them one base, the others up to `max_seg`; a quarter traversed '-', a tenth
    lower case), and a bubble at the repeat's right end: one more copy of the motif, or the link that skips it.  The units
    are joined end to end and closed by one more segment; ids 1.. in path order.  tandem_haplotypes draws the paths."""
    seqs, units, last = _tandem_plan(n_units, seed, max_copies, max_seg)
    v1, s1, v2, s2 = [], [], [], []

    def link(a, b):
        v1.append(a[0] - 1), s1.append(L if a[1] else R), v2.append(b[0] - 1), s2.append(R if b[1] else L)
    for u, (steps, x) in enumerate(units):
        for a, b in zip(steps, steps[1:]):
            link(a, b)
        z = units[u + 1][0][0] if u + 1 < n_units else (last, 0)
        link(steps[-1], (x, 0)), link((x, 0), z), link(steps[-1], z)
    return _mk(np.arange(1, len(seqs) + 1), v1, s1, v2, s2), seqs


def tandem_haplotypes(n_units: int, seed: int, n: int, max_copies: int = 40, max_seg: int = 70) -> Paths:
    """`n` haplotypes of tandem_indels(n_units, seed, ...): each walks the units and takes the extra copy of every bubble with
    probability 1/2 (so the first one, as the reference, sees insertions and deletions alike); PanSN names, one sample a
    haplotype (`hap<k>#1#chr1`)."""
    _, units, last = _tandem_plan(n_units, seed, max_copies, max_seg)
    rng = np.random.default_rng([seed, n])
    pieces = []
    for _ in range(n):
        take = rng.random(n_units) < 0.5
        ids, rev = [], []
        for (steps, x), t in zip(units, take.tolist()):
            ids += [s[0] for s in steps] + ([x] if t else [])
            rev += [s[1] for s in steps] + ([0] if t else [])
        pieces.append((ids + [last], rev + [0]))
    return _paths([f"hap{h}#1#chr1" for h in range(n)], pieces)


def _complex_plan(n_units: int, seed: int):
    """The units of complex_alleles: (sequence of every segment, ids 1.. in path order; per unit the id of its flank and the
    ids of its alleles' segments, 0 for an allele without a base (the link that skips the bubble); the closing segment)."""
    rng = np.random.default_rng([seed, 77])
    seqs, units = [], []

    def seg(text):
        seqs.append(text)
        return len(seqs)

    def draw(n, two):
        return "".join(two[int(k)] if rng.random() < 0.7 else "ACGT"[int(rng.integers(0, 4))] for k in rng.integers(0, 2, size=n))
    for u in range(n_units):
        two = ["AC", "AT", "CG", "GT"][int(rng.integers(0, 4))]
        # unit 0 begins the contig (an empty flank: its record has POS 1) with alleles that differ in a leading run; one unit in
        # sixteen has an empty flank too, so that its skipped allele is an empty text
        bare = u == 0 or rng.random() < 1 / 16
        flank = seg("" if bare else draw(int(rng.integers(2, 7)), "ACGT"[:2]) + "ACGT"[int(rng.integers(0, 4))])
        if u == 0:
            alleles = ["AAC", "AC", "AAAC"]
        else:
            ref = draw(int(rng.integers(1, 11)), two)
            alleles = [ref]
            for _ in range(int(rng.integers(2, 5))):
                b = list(ref)
                for _ in range(int(rng.integers(1, 5))):
                    r, p, k = rng.random(), int(rng.integers(0, len(b) + 1)), int(rng.integers(1, 4))
                    if r < 0.4 and p < len(b):
                        b[p] = draw(1, two)
                    elif r < 0.7:
                        b[p:p] = list(draw(k, two))
                    else:
                        del b[p:p + k]
                alleles.append("".join(b))
            if bare:
                alleles[-1] = ""  # (behind an empty flank the skipped allele is an empty text)
            elif rng.random() < 0.1:
                alleles[-1] = ref.lower()  # (REF's text after upper-casing)
            if rng.random() < 0.1:
                alleles = [a.lower() if k % 2 else a for k, a in enumerate(alleles)]
        ids, seen_empty = [], False
        for a in alleles:
            if a:
                ids.append(seg(a))
            elif not seen_empty:
                ids.append(0)
                seen_empty = True
        units.append((flank, ids))
    return seqs, units, seg(draw(4, "AC"))


def complex_alleles(n_units: int, seed: int):
    """Bubbles of several small edits ("Decomposed calls"): (graph, sequence of every segment).  A unit is a flank of 3 to 7
    bases and a bubble of parallel segments: a REF of 1 to 10 bases over a two-letter-biased alphabet and two to four ALTs
    derived from it by one to four random substitutions, insertions and deletions of one to three bases (an allele that lost
    every base is the link that skips the bubble; a tenth of the units carry REF's text once more in lower case).  Unit 0
    has an empty flank and alleles that differ in a leading run, one later unit in sixteen an empty flank and a skipped allele.  The units are
    joined end to end and closed by one more segment; ids 1.. in path order.  complex_haplotypes draws the paths."""
    seqs, units, last = _complex_plan(n_units, seed)
    v1, s1, v2, s2 = [], [], [], []
    for u, (flank, ids) in enumerate(units):
        z = units[u + 1][0] if u + 1 < n_units else last
        for x in ids:
            if x:
                v1.append(flank - 1), s1.append(R), v2.append(x - 1), s2.append(L)
                v1.append(x - 1), s1.append(R), v2.append(z - 1), s2.append(L)
            else:
                v1.append(flank - 1), s1.append(R), v2.append(z - 1), s2.append(L)
    return _mk(np.arange(1, len(seqs) + 1), v1, s1, v2, s2), seqs


def complex_haplotypes(n_units: int, seed: int, n: int) -> Paths:
    """`n` haplotypes of complex_alleles(n_units, seed): each takes the first allele of a bubble with probability 1/2, else
    one of the others; PanSN names, one sample a haplotype (`hap<k>#1#chr1`)."""
    _, units, last = _complex_plan(n_units, seed)
    rng = np.random.default_rng([seed, n, 78])
    pieces = []
    for _ in range(n):
        ids = []
        for flank, al in units:
            k = 0 if rng.random() < 0.5 else int(rng.integers(1, len(al)))
            ids += [flank] + ([al[k]] if al[k] else [])
        ids.append(last)
        pieces.append((ids, [0] * len(ids)))
    return _paths([f"hap{h}#1#chr1" for h in range(n)], pieces)


_VNTR_UNIT = 5  # segments a loop site: flank, entry, two units, exit
_VNTR_LINKS = [(0, 1), (1, 2), (1, 3), (2, 4), (3, 4), (4, 1), (4, 5)]


def vntr_haplotypes(n_sites: int, n_haps: int, max_copies: int, seed: int, reverse_every: int = 0):
    """Tandem repeats as a graph keeps them ("Untangled calls"): (Links, Paths) of a chain of `n_sites` loop sites and `n_haps`
    haplotypes through it.  Site i has a flank f = 5 i + 1, an entry a = f + 1, the units x = f + 2 and y = f + 3 and an exit
    z = f + 4, with links f>a a>x a>y x>z y>z z>a (the loop) and z > the next flank; a last flank closes the chain.  A
    haplotype walks every site 1 .. `max_copies` times, each copy through a unit chosen at random; every `reverse_every`-th
    haplotype is written walking the chain backwards ('<' steps from the last flank to the first).  PanSN names, one sample a
    haplotype (`hap<k>#1#chr1`); haplotype 0, the reference, walks forwards.  Vectorised over the laps of a haplotype."""
    size = _VNTR_UNIT
    base = size * np.arange(n_sites, dtype=np.int64)[:, None]
    la = np.array(_VNTR_LINKS, dtype=np.int64)
    links = from_plus_links(np.arange(1, size * n_sites + 2, dtype=np.uint32), (base + la[:, 0][None, :]).reshape(-1),
                            (base + la[:, 1][None, :]).reshape(-1))
    rng = np.random.default_rng(seed)
    pieces = []
    for h in range(n_haps):
        copies = rng.integers(1, max_copies + 1, size=n_sites)
        units = rng.integers(0, 2, size=int(copies.sum()))
        site = np.repeat(np.arange(n_sites, dtype=np.int64), copies)  # of every lap
        start = np.zeros(n_sites + 1, dtype=np.int64)  # first step of every site: its flank, then three steps a lap
        np.cumsum(1 + 3 * copies, out=start[1:])
        first_lap = np.cumsum(copies) - copies
        at = start[site] + 1 + 3 * (np.arange(site.size, dtype=np.int64) - first_lap[site])
        w = np.empty(int(start[-1]) + 1, dtype=np.uint32)
        w[start[:-1]] = size * np.arange(n_sites, dtype=np.int64) + 1
        w[at] = size * site + 2
        w[at + 1] = size * site + 3 + units
        w[at + 2] = size * site + 5
        w[-1] = size * n_sites + 1
        if reverse_every and h and h % reverse_every == reverse_every - 1:
            pieces.append((w[::-1].copy(), np.ones(w.size, dtype=np.uint8)))
        else:
            pieces.append((w, np.zeros(w.size, dtype=np.uint8)))
    return links, _paths([f"hap{h}#1#chr1" for h in range(n_haps)], pieces)


def _braid_ids(n_sites: int, layers: int, width: int, seed: int) -> np.ndarray:
    """Segment id of inner segment (site, layer, position) of braid(): a site's inner ids shuffled, so that a walk's segments
    do not ascend."""
    rng = np.random.default_rng(seed)
    m = layers * width
    ids = np.empty((n_sites, m), dtype=np.int64)
    for i in range(n_sites):
        ids[i] = i * (m + 1) + 2 + rng.permutation(m)
    return ids.reshape(n_sites, layers, width)


def braid(n_sites: int, layers: int, width: int, seed: int = 0) -> Links:
    """Sites the PVST does not split further ("Clustered calls"): `n_sites` sites joined end to end, site i between its entry
    segment e = i (layers width + 1) + 1 and the next site's entry, which is its exit.  Between them lie `layers` layers of
    `width` parallel segments, consecutive layers linked completely (no inner flubble exists), the entry to every segment of the
    first layer, every segment of the last layer to the exit, and a deletion link entry > exit.  The inner ids of a site are
    shuffled by `seed` (braid_haplotypes with the same seed walks them)."""
    m = layers * width
    ids = _braid_ids(n_sites, layers, width, seed) - 1  # vertex indices: the ids are 1 .. V
    src, dst = [], []
    for i in range(n_sites):
        e, z = i * (m + 1), (i + 1) * (m + 1)
        src.append(np.array([e])), dst.append(np.array([z]))
        if not layers:
            continue
        src.append(np.full(width, e)), dst.append(ids[i, 0])
        for k in range(layers - 1):
            src.append(np.repeat(ids[i, k], width)), dst.append(np.tile(ids[i, k + 1], width))
        src.append(ids[i, layers - 1]), dst.append(np.full(width, z))
    return from_plus_links(np.arange(1, n_sites * (m + 1) + 2, dtype=np.uint32), np.concatenate(src), np.concatenate(dst))


def braid_haplotypes(n_sites: int, layers: int, width: int, n: int, seed: int = 0, mutate: float = 0.05, skip: float = 0.05,
                     reverse_every: int = 0) -> Paths:
    """`n` haplotypes of braid(n_sites, layers, width, seed), near-equal as the haplotypes of a population are: every site has a
    base walk (a segment of every layer), and a haplotype takes the deletion link with probability `skip`, else the base walk
    with every layer's segment redrawn with probability `mutate`.  Every `reverse_every`-th haplotype is written walking
    backwards.  PanSN names, one sample a haplotype (`hap<k>#1#chr1`); haplotype 0 is the reference."""
    m = layers * width
    ids = _braid_ids(n_sites, layers, width, seed)
    rng = np.random.default_rng(seed + 1)
    base = rng.integers(0, max(width, 1), size=(n_sites, layers))
    entry = np.arange(n_sites + 1, dtype=np.int64) * (m + 1) + 1
    pieces = []
    for h in range(n):
        gone = rng.random(n_sites) < skip
        pick = np.where(rng.random((n_sites, layers)) < mutate, rng.integers(0, max(width, 1), size=(n_sites, layers)), base)
        w = [np.array([1], dtype=np.int64)]
        for i in range(n_sites):
            if not gone[i] and layers:
                w.append(ids[i, np.arange(layers), pick[i]])
            w.append(entry[i + 1:i + 2])
        w = np.concatenate(w).astype(np.uint32)
        if reverse_every and h and h % reverse_every == reverse_every - 1:
            pieces.append((w[::-1].copy(), np.ones(w.size, dtype=np.uint8)))
        else:
            pieces.append((w, np.zeros(w.size, dtype=np.uint8)))
    return _paths([f"hap{h}#1#chr1" for h in range(n)], pieces)

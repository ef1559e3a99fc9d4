"""Plain-Python restatement of the flubble traversals ("Flubble traversals"), the yardstick of
povu_hip_forest_traversals.

A path is a list of steps (segment id, orientation), orientation 0 = '>' (GFA '+'), 1 = '<' (GFA '-').  A query is the
pair of boundary steps (S, Z) of a PVST vertex, numbered like the walks' queries (walks_ref.queries_of_arrays).

Forward scan: from every position i with p[i] == S, the first later position j whose segment is one of the two boundary
segments closes the scan; p[i..j] is a traversal (strand '+') when p[j] == Z and j - i + 1 <= max_steps.  Reverse scan:
the same from p[i] == flip(Z), closing only on flip(S); its sequence is read backwards with every orientation flipped
(strand '-').  A scan that meets the other boundary step sets STRAY, one that would need more than max_steps steps (the
path still goes on at i + max_steps) sets LONG, one that reaches the end of the path sets OPEN.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

LONG, STRAY, OPEN = 1, 2, 4
DEFAULT_MAX_STEPS = 65536

Step = Tuple[int, int]


def flip(s: Step) -> Step:
    return (s[0], 1 - s[1])


class PathIndex:
    """The paths and, per path, the positions of every step value (so that a query looks at its starts only)."""

    def __init__(self, paths: Sequence[Sequence[Step]]):
        self.paths = [[(int(a), int(b)) for a, b in p] for p in paths]
        self.at: List[Dict[Step, List[int]]] = []
        for p in self.paths:
            d: Dict[Step, List[int]] = {}
            for i, s in enumerate(p):
                d.setdefault(s, []).append(i)
            self.at.append(d)


def _scan(p, i, close, b1, b2, max_steps):
    """(j, 0) when the scan from position i closes at j, else (None, the status bit that ends it)."""
    for j in range(i + 1, len(p)):
        if j - i + 1 > max_steps:
            return None, LONG
        if p[j][0] == b1 or p[j][0] == b2:
            return (j, 0) if p[j] == close else (None, STRAY)
    return None, OPEN


def traversals_of(index: PathIndex, s: Step, z: Step, max_steps: int = DEFAULT_MAX_STEPS):
    """(alleles, traversals, status) of one query.  alleles: list of step lists (S -> Z); traversals: list of
    (path, first, last, reverse 0/1, allele), ordered by (path, first)."""
    if s[0] == z[0]:
        return [], [], 0
    status, found = 0, []
    for pi, p in enumerate(index.paths):
        starts = [(i, 0) for i in index.at[pi].get(s, [])] + [(i, 1) for i in index.at[pi].get(flip(z), [])]
        for i, rev in sorted(starts):
            j, bit = _scan(p, i, flip(s) if rev else z, s[0], z[0], max_steps)
            status |= bit
            if j is not None:
                seq = p[i:j + 1]
                if rev:
                    seq = [flip(x) for x in reversed(seq)]
                found.append((pi, i, j, rev, tuple(seq)))
    alleles: List[tuple] = []
    num: Dict[tuple, int] = {}
    travs = []
    for pi, i, j, rev, seq in found:
        if seq not in num:
            num[seq] = len(alleles)
            alleles.append(seq)
        travs.append((pi, i, j, rev, num[seq]))
    return [list(a) for a in alleles], travs, status


def flat(index: PathIndex, queries, max_steps: int = DEFAULT_MAX_STEPS):
    """The arrays povu_hip_forest_traversals returns, for `queries` [(S, Z), ...]."""
    trav_off, allele_off, status = [0], [0], []
    path, first, last, rev, allele = [], [], [], [], []
    step_off, step_id, step_or = [0], [], []
    for s, z in queries:
        al, tr, st = traversals_of(index, s, z, max_steps)
        status.append(st)
        for pi, i, j, r, a in tr:
            path.append(pi), first.append(i), last.append(j), rev.append(r), allele.append(a)
        for a in al:
            step_id += [x[0] for x in a]
            step_or += [x[1] for x in a]
            step_off.append(len(step_id))
        trav_off.append(len(path))
        allele_off.append(len(step_off) - 1)
    u32 = lambda x: np.array(x, dtype=np.uint32)  # noqa: E731
    return dict(trav_off=np.array(trav_off, np.uint64), allele_off=np.array(allele_off, np.uint64),
                status=np.array(status, np.uint8), path=u32(path), first=u32(first), last=u32(last),
                allele=u32(allele), reverse=np.array(rev, np.uint8), step_off=np.array(step_off, np.uint64),
                step_id=u32(step_id), step_or=np.array(step_or, np.uint8))


def paths_from_arrays(off, ids, rev) -> List[List[Step]]:
    """Step lists from the flat (u64 offsets, u32 ids, u8 rev) form (workloads.Paths)."""
    off, ids, rev = np.asarray(off).tolist(), np.asarray(ids).tolist(), np.asarray(rev).tolist()
    return [list(zip(ids[off[k]:off[k + 1]], rev[off[k]:off[k + 1]])) for k in range(len(off) - 1)]


def as_text(seq) -> str:
    return "".join((">" if o == 0 else "<") + str(i) for i, o in seq)

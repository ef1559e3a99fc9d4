"""Plain-Python restatement of the flubble walks ("Flubble walks"), the yardstick of povu_hip_forest_walks.

A step is (segment id, orientation), orientation 0 = '>' (leaves through the r side), 1 = '<' (leaves through the l side).
A link from the exit side to side y of u gives the step (u, 0) when y is l, (u, 1) when y is r -- so the orientation of
the next step is the side it enters by.  Successors are tried by ascending (id, orientation); parallel links count once.
"""
from __future__ import annotations

import re
from typing import Dict, List, Sequence, Tuple

import numpy as np

MORE, LONG, BUDGET = 1, 2, 4
DEFAULTS = dict(max_walks=64, max_steps=1000, max_expansions=65536)

Step = Tuple[int, int]


def successors(links) -> Dict[Tuple[int, int], List[Step]]:
    """(segment id, exit side) -> sorted, de-duplicated list of next steps; from a workloads.Links record."""
    vid = np.asarray(links.vid).tolist()
    out: Dict[Tuple[int, int], set] = {}
    for a, sa, b, sb in zip(np.asarray(links.v1).tolist(), np.asarray(links.s1).tolist(), np.asarray(links.v2).tolist(),
                            np.asarray(links.s2).tolist()):
        out.setdefault((vid[a], sa), set()).add((vid[b], sb))
        out.setdefault((vid[b], sb), set()).add((vid[a], sa))
    return {k: sorted(v) for k, v in out.items()}


def walks_of(succ, start: Step, end: Step, max_walks=64, max_steps=1000, max_expansions=65536):
    """(walks, status) of one query: every walk a list of (id, orientation) from `start` to `end`."""
    K, L, E = max_walks, max_steps, max_expansions
    if start[0] == end[0]:
        return [], 0
    if L <= 1:
        return [], LONG
    status, exp, walks = 0, 0, []
    stack = [[start, 0]]  # (step, next successor to try)
    on_path = {start[0]}
    while stack:
        step, i = stack[-1]
        cand = succ.get((step[0], 1 - step[1]), ())
        nxt = None
        while i < len(cand):
            c = cand[i]
            i += 1
            if c[0] == end[0]:
                if c == end:
                    nxt = c
                    break
                continue  # Z's segment the other way round: no walk passes through it
            if c[0] in on_path:
                continue
            nxt = c
            break
        stack[-1][1] = i
        if nxt is None:
            stack.pop()
            on_path.discard(step[0])
            continue
        if exp == E:
            status |= BUDGET
            break
        exp += 1
        if nxt == end:
            if len(walks) == K:
                status |= MORE
                break
            walks.append([s for s, _ in stack] + [end])
            continue
        if len(stack) + 1 >= L:
            status |= LONG
            continue
        stack.append([nxt, 0])
        on_path.add(nxt[0])
    return walks, status


def queries_of_arrays(a_id, a_or, z_id, z_or) -> List[Tuple[Step, Step]]:
    """Queries of one PVST (arrays indexed by PVST vertex, entry 0 = the root, skipped)."""
    return [((int(a_id[v]), int(a_or[v])), (int(z_id[v]), int(z_or[v]))) for v in range(1, len(a_id))]


_LABEL = re.compile(r"^([<>])(\d+)([<>])(\d+)$")


def queries_of_pvst_text(text: str) -> List[Tuple[Step, Step]]:
    """Queries of a PVST file: every vertex line but the root (D), in file order; the route letter is ignored."""
    out = []
    for line in text.splitlines():
        f = line.split("\t")
        if f[0] in ("H", "D") or len(f) < 3:
            continue
        m = _LABEL.match(f[2])
        if not m:
            raise ValueError(f"bad PVST label {f[2]!r}")
        out.append(((int(m.group(2)), 0 if m.group(1) == ">" else 1), (int(m.group(4)), 0 if m.group(3) == ">" else 1)))
    return out


def flat(succ, queries: Sequence[Tuple[Step, Step]], **caps):
    """The arrays povu_hip_forest_walks returns: walk_off, step_off, step_id, step_or, status (numpy)."""
    c = dict(DEFAULTS, **caps)
    walk_off, step_off, ids, ors, status = [0], [0], [], [], []
    for s, z in queries:
        ws, st = walks_of(succ, s, z, **c)
        for w in ws:
            ids += [x for x, _ in w]
            ors += [o for _, o in w]
            step_off.append(len(ids))
        walk_off.append(len(step_off) - 1)
        status.append(st)
    return dict(walk_off=np.array(walk_off, np.uint32), step_off=np.array(step_off, np.uint32),
                step_id=np.array(ids, np.uint32), step_or=np.array(ors, np.uint8), status=np.array(status, np.uint8))


def as_text(walk: Sequence[Step]) -> str:
    """'>1>2<3' form of a walk (for readable test answers)."""
    return "".join((">" if o == 0 else "<") + str(i) for i, o in walk)

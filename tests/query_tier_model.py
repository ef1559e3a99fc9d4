"""The tiering of the walks and the traversals, restated (povu_amd/csrc/hip/walk_rules.hpp, walk_kernels.hip, trav_kernels.hip):
which query or task tier 1 hands over, how many lanes tier 2 gets, whether the successors are sorted by the radix path, and what
a search does to the path set of its tier-2 lane.  The answers themselves stay with walks_ref.py and traversals_ref.py: nothing
here yields a walk or a traversal.  tests/test_query_tier_inputs.py holds the constants to the sources and the cases of
tests/query_tier_cases.py to these figures; tests/test_gpu_query_tiers.py holds n_tier2 of the device to them."""
from __future__ import annotations

import numpy as np

import traversals_ref as TR

T1_DEPTH = 16          # frames of a tier-1 stack
T1_EXPANSIONS = 4096   # expansions tier 1 spends before it hands a query over
SORT_IN_LANE = 64      # a side of more slots sends the successors through the radix sort
T2_MAX_LANES = 16384
T2_SCRATCH = 256 << 20
MAX_STEPS_CAP = 1 << 24
T1_STEPS = 64          # path steps tier 1 of the traversals looks at
HASH = 2654435761
MORE, LONG, BUDGET = 1, 2, 4


def bits_for(max_value: int) -> int:
    b = 1
    while b < 32 and (1 << b) <= max_value:
        b += 1
    return b


def tbits_of(max_steps: int) -> int:
    return max(4, bits_for(2 * max_steps - 1))


def t2_lanes(n2: int, max_steps: int) -> int:
    """lanes of the walks' tier 2: one per query handed over, at most 16384 and 256 MiB of scratch"""
    if not n2:
        return 0
    lane_words = 2 * max_steps + (1 << tbits_of(max_steps))
    return max(1, min(n2, T2_MAX_LANES, T2_SCRATCH // (lane_words * 4)))


def max_side_slots(g) -> int:
    sides = np.concatenate([g.v1.astype(np.int64) * 2 + g.s1, g.v2.astype(np.int64) * 2 + g.s2])
    return int(np.bincount(sides).max()) if len(sides) else 0


def has_hub(g) -> bool:
    return max_side_slots(g) > SORT_IN_LANE


class PathSet:
    """The open-addressed set of a tier-2 lane with its four events counted: a probe that wraps past the last slot, an entry a
    deletion leaves in place, one it moves, one it moves across the wrap."""

    def __init__(self, tbits: int):
        self.tbits, self.n = tbits, 1 << tbits
        self.t = [0] * self.n
        self.wrap_probe = self.stayed = self.moved = self.shift_across = 0
        self.max_load = 0

    def home(self, u: int) -> int:
        return ((u * HASH) & 0xFFFFFFFF) >> (32 - self.tbits)

    def _next(self, i: int) -> int:
        if i + 1 == self.n:
            self.wrap_probe += 1
            return 0
        return i + 1

    def push(self, u: int) -> None:
        i = self.home(u)
        while self.t[i]:
            i = self._next(i)
        self.t[i] = u + 1
        self.max_load = max(self.max_load, sum(1 for x in self.t if x))

    def pop(self, u: int) -> None:
        hole = self.home(u)
        while self.t[hole] != u + 1:
            hole = self._next(hole)
        j = (hole + 1) % self.n
        while self.t[j]:
            h = self.home(self.t[j] - 1)
            if 1 <= (h - hole) % self.n <= (j - hole) % self.n:  # its home lies in (hole, j]: it stays
                self.stayed += 1
            else:
                self.moved += 1
                self.shift_across += j < hole
                self.t[hole] = self.t[j]
                hole = j
            j = (j + 1) % self.n
        self.t[hole] = 0

    def on_path(self, u: int) -> bool:
        i = self.home(u)
        while self.t[i]:
            if self.t[i] == u + 1:
                return True
            i = self._next(i)
        return False

    def events(self):
        return dict(wrap_probe=self.wrap_probe, stayed=self.stayed, moved=self.moved, shift_across=self.shift_across,
                    max_load=self.max_load)


def search(succ, s, z, max_walks=64, max_steps=1000, max_expansions=65536, tier1=False, path_set=None, index_of=None):
    """The search of one query as dfs runs it, figures only: frames (the deepest stack), expansions spent, status, and -- with
    tier1 -- whether tier 1's limits end it (handover: a 17th frame, or an expansion after min(E, 4096), before the search ends
    otherwise).  path_set / index_of: a PathSet that is pushed and popped as a tier-2 lane's is, vertex indices from index_of."""
    K, L, E = max_walks, max_steps, max_expansions
    out = dict(frames=0, expansions=0, status=0, walks=0, handover=False)
    if s[0] == z[0]:
        return out
    if L <= 1:
        out["status"] = LONG
        return out
    ecap = min(E, T1_EXPANSIONS) if tier1 else E
    cap = T1_DEPTH if tier1 else L

    def push(step):
        if path_set is not None:
            path_set.push(index_of[step[0]])

    def pop(step):
        if path_set is not None:
            path_set.pop(index_of[step[0]])

    stack = [[s, 0]]
    on = {s[0]}
    push(s)
    out["frames"] = 1
    exp = 0
    while stack:
        step, i = stack[-1]
        cand = succ.get((step[0], 1 - step[1]), ())
        nxt = None
        while i < len(cand):
            c = cand[i]
            i += 1
            if c[0] == z[0]:
                if c == z:
                    nxt = c
                    break
                continue
            if path_set is not None:
                assert path_set.on_path(index_of[c[0]]) == (c[0] in on)
            if c[0] in on:
                continue
            nxt = c
            break
        stack[-1][1] = i
        if nxt is None:
            stack.pop()
            on.discard(step[0])
            pop(step)
            continue
        if exp == E:
            out["status"] |= BUDGET
            break
        if exp == ecap:
            out["handover"] = True
            break
        exp += 1
        if nxt == z:
            if out["walks"] == K:
                out["status"] |= MORE
                break
            out["walks"] += 1
            continue
        if len(stack) + 1 >= L:
            out["status"] |= LONG
            continue
        if len(stack) == cap:
            out["handover"] = True
            break
        stack.append([nxt, 0])
        on.add(nxt[0])
        push(nxt)
        out["frames"] = max(out["frames"], len(stack))
    out["left_on_path"] = len(stack)  # (what the unwinding loop takes off the path set)
    while stack:
        pop(stack.pop()[0])
    if path_set is not None:
        assert not any(path_set.t)
    out["expansions"] = exp
    return out


def walks_n_tier2(succ, queries, **caps) -> int:
    """queries tier 1 of the walks hands over"""
    return sum(search(succ, s, z, tier1=True, **caps)["handover"] for s, z in queries)


# ---- traversals

def trav_tasks(paths, queries, max_steps=TR.DEFAULT_MAX_STEPS):
    """[(query, path, position, reverse, handed over)] of every scan: a step equal to S starts a forward scan, one equal to
    flip(Z) a reverse scan.  Tier 1 hands a scan over iff none of the offsets 1 .. 64 is on a boundary segment and the window --
    min(path end, position + max_steps) -- goes on past offset 65."""
    at = {}
    for pi, p in enumerate(paths):
        for i, st in enumerate(p):
            at.setdefault((int(st[0]), int(st[1])), []).append((pi, i))
    out = []
    for q, (s, z) in enumerate(queries):
        if s[0] == z[0]:
            continue
        for start, rev in ((s, 0), (TR.flip(z), 1)):
            for pi, i in at.get(start, ()):
                p = paths[pi]
                lim = min(len(p), i + max_steps)
                near = any(p[j][0] in (s[0], z[0]) for j in range(i + 1, min(lim, i + 1 + T1_STEPS)))
                out.append((q, pi, i, rev, (not near) and lim > i + 1 + T1_STEPS))
    return out


def trav_n_tier2(paths, queries, max_steps=TR.DEFAULT_MAX_STEPS) -> int:
    return sum(t[4] for t in trav_tasks(paths, queries, max_steps))

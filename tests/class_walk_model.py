"""Restatement of the two class walks of the tree stage (tree_kernels.hip sections 5 and 6, walk_step.inc) with telemetry.
Plain Python, no GPU.  It shares steps (1), (2), (4), (5) with the model of test_parallel_tree_model.py and replaces step (3),
the DFS inside a class, by two literal simulations:

  small_walk   k_class_dfs_small, one lane: batches of four slots, the black follow-through that pushes two levels, the
               DFS_STK levels of scan state in LDS and the resumption from dps / loff below them, the budget test.
  wave_walk    k_class_walk_wave<false> as POVU_HIP_WALK_ROUTE=2 runs it: candidate records (k_class_recs), looks of 64 lanes,
               the push rule, the ring of 64 with its eviction of 32 into doubling chunks, the pop.  Ring and chunks are kept
               as arrays and every entry read back is compared with the logical stack.

Both must leave the same DFS parents as the reference's lexicographic DFS; model_graph() checks them against each other and
finish_tree() turns them into the tree the oracle's dump is compared with.  Only `dist` and `probe` see the vertex numbering.
The forms with the window (routes 0 and 1) are not simulated: their pushes depend on the window's position."""
from test_parallel_tree_model import class_setup, component_dumps, finish_tree, walk_class

CLASS_BUDGET, BUDGET_FLOOR = 256, 16
DFS_STK = 8
W_INLINE = 6
W_CHUNK0 = 64
W_WIN, W_WIN_BACK = 128, 16
W_PROBE, W_TRIAL = 48, 512


def chunk_of(d):
    """wstk_addr: chunk 0 holds entries [0, 64), chunk c >= 1 the entries [64 << (c - 1), 64 << c)."""
    return 0 if d < W_CHUNK0 else (d // W_CHUNK0).bit_length()


def chunk_size(c):
    return W_CHUNK0 << (c - 1) if c else W_CHUNK0


def candidates(st, S):
    """k_class_recs: the scan list of S filtered down to its own class, in record order (black edge first)."""
    ecc = st["ecc"]
    return [(o, slot) for o, _, slot in st["scan"](S) if o != S and ecc[o] == ecc[S]]


def small_walk(st, cls, s, budget=None):
    """k_class_dfs_small on the class entered at s.  Writes dpar / cslot; returns the telemetry.  budget=None: never abandoned."""
    adj, ecc, dpar, cslot = st["adj"], st["ecc"], st["dpar"], st["cslot"]
    vis = {s}
    dps = {}
    stk = [None] * DFS_STK
    path = []  # (side, first depth of the follow-through pair that pushed it, or None): telemetry only
    t = dict(steps=0, over=False, batches=set(), returns=[], pairs=set(), max_depth=0, adj_end=False)
    u, k, n, sides, depth = s, 0, len(adj[s]), 0, 0
    while True:
        adv = False
        while k <= n:
            rem = n + 1 - k
            first = k - 1 if k else 0  # the 16-byte load covers ladj[lo + first .. + 4)
            if st["goff"][u] + first + 4 > st["adj_words"]:
                t["adj_end"] = True
            slots = [u ^ 1 if (k + i) == 0 else adj[u][k + i - 1][0] for i in range(min(rem, 4))]
            j = next((i for i, o in enumerate(slots) if ecc[o] == cls and o not in vis), 4)
            t["batches"].add((min(rem, 4), j))
            if j == 4:
                k += min(rem, 4)
                continue
            o, slot = slots[j], k + j
            k = slot + 1
            if depth < DFS_STK:
                stk[depth] = (u, k, n)
            path.append((u, None))
            depth += 1
            sides += 1
            p = o ^ 1
            vis.add(o)
            dpar[o], cslot[o] = u, slot
            dps[o] = (u, slot)
            if slot != 0 and p not in vis and ecc[p] == cls:  # the black follow-through: two levels at once
                vis.add(p)
                dpar[p], cslot[p] = o, 0
                dps[p] = (o, 0)
                t["pairs"].add(depth - 1)
                if depth < DFS_STK:
                    stk[depth] = (o, 1, len(adj[o]))
                path.append((o, depth - 1))
                depth += 1
                sides += 1
                u = p
            else:
                u = o
            n = len(adj[u])
            k = 1
            adv = True
            break
        t["max_depth"] = max(t["max_depth"], depth)
        if adv:
            t["steps"] = sides
            if budget is not None and sides > budget:
                t["over"] = True
                return t
            continue
        if u == s:
            return t
        depth -= 1
        want, pair = path.pop()
        if depth < DFS_STK:
            u, k, n = stk[depth]
        else:
            up = dps[u]
            u, k, n = up[0], up[1] + 1, len(adj[up[0]])
        assert u == want
        more = any(ecc[o] == cls and o not in vis for o, _ in adj[u][k - 1:]) if k >= 1 else True
        t["returns"].append(dict(depth=depth, lds=depth < DFS_STK, scans=k <= n, advances=more, pair_first=pair))


def wave_walk(st, cls, s, cand):
    """The plain wave walk (route 2) on the class entered at s.  Writes dpar / cslot; returns the telemetry."""
    dpar, cslot = st["dpar"], st["cslot"]
    vis = {s}
    ring = [None] * 64
    hbm = {}  # chunk -> list
    stack = []  # the logical stack, for the cross-check
    depth = lds_lo = n_chunks = 0
    evicted = set()
    t = dict(max_entries=0, resumes=[], final_drop=None, pool=0, re_evictions=0, looks=set(), look_moves=set(), beyond_only_pushes=0, steps=0)

    def addr(d):
        c = chunk_of(d)
        return c, d - (chunk_size(c) if c else 0)

    def push(side, jn):
        nonlocal depth, lds_lo, n_chunks
        if depth - lds_lo == 64:
            ev = lds_lo
            if ev + 32 > (W_CHUNK0 << (n_chunks - 1) if n_chunks else 0):
                sz = chunk_size(n_chunks)
                hbm[n_chunks] = [None] * sz
                t["pool"] += sz
                n_chunks += 1
            for l in range(32):
                c, off = addr(ev + l)
                assert c < n_chunks and off < len(hbm[c]), "eviction outside the chunks taken"
                hbm[c][off] = ring[(ev + l) & 63]
            if any(ev + l in evicted for l in range(32)):  # (entries fetched back and pushed on past: the same values again)
                t["re_evictions"] += 1
            evicted.update(range(ev, ev + 32))
            lds_lo = ev + 32
        ring[depth & 63] = (side, jn)
        stack.append((side, jn))
        depth += 1
        t["max_entries"] = max(t["max_entries"], depth)

    u, j0 = s, 0
    pend = None
    resumed = None
    moved = 0  # looks of 64 the scan of u has moved on by since it arrived or resumed there
    while True:
        lst = cand[u]
        n = len(lst)
        look = lst[j0:j0 + 64]
        m = [i for i, (o, _) in enumerate(look) if o not in vis]
        if pend is not None:  # the bookkeeping of the black step, carried out behind this step's loads
            if pend[1]:
                push(pend[0], 1)
            pend = None
        beyond = j0 + 64 < n
        t["looks"].add((n, j0))
        if resumed is not None and (m or not beyond):
            resumed["first_open"] = j0 + m[0] if m else None
            resumed = None
        if m:
            f = m[0]
            child, slot = look[f]
            if len(m) > 1 or beyond:
                t["beyond_only_pushes"] += len(m) == 1
                push(u, j0 + f + 1)
            if moved:
                t["look_moves"].add(moved)
            moved = 0
            vis.add(child)
            dpar[child], cslot[child] = u, slot
            t["steps"] += 1
            cl = cand[child]
            if cl and cl[0][0] == child ^ 1 and (child ^ 1) not in vis:
                pend = (child, len(cl) > 1)
                vis.add(child ^ 1)
                dpar[child ^ 1], cslot[child ^ 1] = child, 0
                t["steps"] += 1
                u = child ^ 1
            else:
                u = child
            j0 = 0
            continue
        if beyond:
            j0 += 64
            moved += 1
            continue
        if moved:
            t["look_moves"].add(moved)
        moved = 0
        before, fetches = depth, 0
        while True:
            if depth == 0:
                t["final_drop"] = dict(dropped=before, fetches=fetches)
                assert not stack
                return t
            fetched = False
            if lds_lo >= depth:
                cnt = min(depth, 64)
                for l in range(cnt):
                    d = depth - 1 - l
                    c, off = addr(d)
                    ring[d & 63] = hbm[c][off]
                lds_lo = depth - cnt
                fetches += 1
                fetched = True
            cnt = depth - lds_lo
            assert 1 <= cnt <= 64
            hit = None
            for l in range(cnt):
                d = depth - 1 - l
                assert ring[d & 63] == stack[d], "the ring / chunk arithmetic lost an entry"
                eu, ej = ring[d & 63]
                el = cand[eu]
                if len(el) > W_INLINE or any(o not in vis for o, _ in el[ej:]):
                    hit = l
                    break
            if hit is None:
                depth -= cnt
                del stack[depth:]
                continue
            depth -= hit + 1
            u, j0 = stack[depth]
            del stack[depth:]
            lds_lo = min(lds_lo, depth)
            resumed = dict(index=depth, dropped=before - depth, fetches=fetches, from_hbm=fetched,
                           chunk=chunk_of(depth) if fetched else None,
                           span=fetched and chunk_of(depth + hit) != chunk_of(depth + hit + 1 - cnt), list_len=len(cand[u]), j=j0)
            t["resumes"].append(resumed)
            break


def probe(cand, s):
    """The form choice of route 0: W_PROBE hops from the entry; (near, tot, hot)."""
    near = tot = 0
    x = s
    for _ in range(W_PROBE):
        lst = cand[x]
        y = None if not lst else (lst[0][0] if lst[0][0] != x ^ 1 else (lst[1][0] if len(lst) > 1 else None))
        if y is None:
            break
        tot += 1
        near += 1 if abs(y - x) <= 64 else 0
        x = y ^ 1
    return near, tot, tot == W_PROBE and 4 * near >= 3 * tot


def model_component(d, tips, base=0, goff0=0, adj_words=None):
    """Tree and telemetry of one component.  base: device index of its side 0 (the side ids of the telemetry are the device's);
    goff0 / adj_words: where its adjacency lists start in the graph's array and how long that array is."""
    st = class_setup(d, tips)
    adj, n = st["adj"], st["n"]
    goff, o = [], goff0
    for S in range(n):
        goff.append(o)
        o += len(adj[S])
    st["goff"], st["adj_words"] = goff, adj_words if adj_words is not None else o
    cand = [candidates(st, S) for S in range(n)]
    members = {}
    for S in range(n):
        members.setdefault(st["ecc"][S], []).append(S)
    classes = []
    for cls, s in sorted(st["entry"].items(), key=lambda kv: kv[1]):
        mem = members[cls]
        if len(mem) < 2:
            continue
        save = (st["dpar"][s], st["cslot"][s])
        # the lane's attempt under either budget: what an abandoned lane wrote is overwritten below, as the wave walk does
        tried = {b: small_walk(st, cls, s, budget=b) for b in (CLASS_BUDGET, BUDGET_FLOOR)}
        walk_class(st, cls, s)
        want = {S: (st["dpar"][S], st["cslot"][S]) for S in mem}
        sm = small_walk(st, cls, s)
        assert {S: (st["dpar"][S], st["cslot"][S]) for S in mem} == want, "small walk differs from the lexicographic DFS"
        wv = wave_walk(st, cls, s, cand)
        # (the wave walk leaves the parent; k_walk_finish finds the slot: the black edge or the first link that leads there)
        assert {S: (st["dpar"][S], st["cslot"][S]) for S in mem} == want, "wave walk differs from the lexicographic DFS"
        assert (st["dpar"][s], st["cslot"][s]) == save
        near, tot, hot = probe(cand, s)
        order = []  # tree steps (parent, child) in walk order = pre-order with children by scan slot
        kids = {}
        for S in mem:
            if S != s:
                kids.setdefault(st["dpar"][S], []).append((st["cslot"][S], S))
        stack = [s]
        while stack:
            x = stack.pop()
            if x != s:
                order.append((base + st["dpar"][x], base + x))
            for _, c in sorted(kids.get(x, []), reverse=True):
                stack.append(c)
        assert len(order) == len(mem) - 1
        classes.append(dict(entry=base + s, sides=len(mem), lo=base + min(mem), hi=base + max(mem), steps=sm["steps"], small=sm, wave=wv,
                            lists={base + S: len(cand[S]) for S in mem}, max_list=max(len(cand[S]) for S in mem),
                            probe=(near, tot), probe_hot=hot, tree_steps=order, dist=[c - p for p, c in order],
                            over={b: tried[b]["over"] for b in tried},
                            abandoned_at={b: (tried[b]["steps"], len(tried[b]["returns"])) for b in tried if tried[b]["over"]}))
        for b in tried:  # (the literal test after each advance and the closed form agree)
            assert tried[b]["over"] == (sm["steps"] > b)
    return finish_tree(st), classes


def model_graph(g, tips=None, max_comp=64):
    """Every component of g: [(rank, dump, tree)], and the classes of more than one side of all of them.  Side indices in the
    telemetry are the device's: components in rank order, 2 * (vertices in front) + local side."""
    dumps = list(component_dumps(g, tips, max_comp))
    adj_words = sum(2 * len(d["ev1"]) - sum(1 for a, sa, b, sb in zip(d["ev1"], d["es1"], d["ev2"], d["es2"]) if a == b and sa == sb)
                    for _, d, _ in dumps)
    comps, classes, base, goff = [], [], 0, 0
    for comp, d, tp in dumps:
        if len(d["gid"]) == 0:
            comps.append((comp, d, None))
        else:
            tree, cl = model_component(d, tp, base, goff, adj_words)
            comps.append((comp, d, tree))
            for c in cl:
                c["comp"] = comp
            classes += cl
        base += 2 * len(d["gidx"])
        goff += 2 * len(d["ev1"]) - sum(1 for a, sa, b, sb in zip(d["ev1"], d["es1"], d["ev2"], d["es2"]) if a == b and sa == sb)
    return comps, classes


def n_over(classes, budget=CLASS_BUDGET):
    return sum(1 for c in classes if c["over"][budget])


def pool_sum(classes, budget=None):
    """PW_POOL_TOP under route 2: every class (budget None: F_BIG_CLASS_DFS) or those the lane handed over."""
    return sum(c["wave"]["pool"] for c in classes if budget is None or c["over"][budget])

"""Pure-numpy model of the device minimum cut (csrc/pfdr_mincut.hip): the
synchronous push-relabel round (push against a snapshot, apply, relabel AFTER
the apply), first phase only, with periodic exact relabelling.

``side="sink"`` is the library's scheme: the preflow starts from the cut's
sink over the reversed network, so the nodes that can still reach the
preflow's sink are those reachable from the cut's source: the smallest
source side, Boykov-Kolmogorov's answer.  ``side="source"`` runs the same
rounds forward and gives the largest source side instead.
``relabel_after_apply=False`` relabels from the residuals before the round's
pushes, the mistake the kernel's comment warns of.
"""
import numpy as np

BOTH, FORWARD = 0, 1


def _arcs(V, Eu, Ev):
    """out[v] = slots a = 2e + side whose tail is v, ascending; head[a]"""
    E = len(Eu)
    head = np.empty(2 * E, np.int64)
    head[0::2], head[1::2] = Ev, Eu
    tail = np.empty(2 * E, np.int64)
    tail[0::2], tail[1::2] = Eu, Ev
    out = [[] for _ in range(V)]
    for a in range(2 * E):
        out[tail[a]].append(a)
    return out, head


def _bfs(V, out, head, ex, res):
    """exact distances to the nodes of negative excess; V where none"""
    h = np.where(ex < 0, 0, -1)
    level = 0
    while True:
        lab = [v for v in range(V) if h[v] == -1
               and any(res[a] > 0 and h[head[a]] == level for a in out[v])]
        if not lab:
            break
        h[lab] = level + 1
        level += 1
    h[h == -1] = V
    return h


def mincut_model(V, Eu, Ev, tr_cap, r_cap, arcs, side="sink", relabel_after_apply=True,
                 period=8, max_rounds=100000, invalid=None):
    """-> (segment uint8[V], rounds); ``invalid`` (a list) receives, per round,
    the number of residual arcs u -> v with h(u) > h(v) + 1 among live nodes
    (a valid labelling has none)"""
    tr = np.asarray(tr_cap, np.float64)
    rc = np.asarray(r_cap, np.float64)
    E = len(Eu)
    out, head = _arcs(V, Eu, Ev)
    res = np.zeros(2 * E)
    if side == "sink":   # reversed network: slot a carries the original arc a ^ 1
        ex = -tr
        res[1::2] = rc
        res[0::2] = rc if arcs == BOTH else 0.0
    else:
        ex = tr.copy()
        res[0::2] = rc
        res[1::2] = rc if arcs == BOTH else 0.0
    h = _bfs(V, out, head, ex, res)
    rounds = 0
    while any(ex[v] > 0 and h[v] < V for v in range(V)):
        if rounds >= max_rounds:
            raise RuntimeError("model: no convergence")
        # push against the snapshot
        delta = np.zeros(2 * E)
        pushed = np.zeros(V, bool)
        for u in range(V):
            rem = ex[u]
            if not (rem > 0 and h[u] < V):
                continue
            for a in out[u]:
                if rem > 0 and res[a] > 0 and h[u] == h[head[a]] + 1:
                    d = min(rem, res[a])
                    delta[a] = d
                    rem -= d
                    pushed[u] = True
        # apply, then relabel
        active = (ex > 0) & (h < V)
        old = res.copy()
        for a in range(2 * E):
            if delta[a] > 0:
                res[a] -= delta[a]
                res[a ^ 1] += delta[a]
        hn = h.copy()
        for u in range(V):
            for a in out[u]:
                ex[u] -= delta[a]
            for a in out[u]:
                ex[u] += delta[a ^ 1]
            if active[u] and not pushed[u]:
                r = res if relabel_after_apply else old
                c = [h[head[a]] + 1 for a in out[u] if r[a] > 0]
                hn[u] = min(min(c), V) if c else V
        h = hn
        rounds += 1
        if invalid is not None:
            invalid.append(sum(1 for u in range(V) if h[u] < V for a in out[u]
                               if res[a] > 0 and h[u] > h[head[a]] + 1))
        if rounds % period == 0:
            h = _bfs(V, out, head, ex, res)
    h = _bfs(V, out, head, ex, res)
    reach = h < V
    # sink side: reached = can reach the preflow's sink = reachable from the
    # cut's source.  source side: reached = can reach the cut's sink.
    seg = np.where(reach, 0, 1) if side == "sink" else np.where(reach, 1, 0)
    return seg.astype(np.uint8), rounds

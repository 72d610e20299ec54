"""Cases for awr_hands_assign (csrc/awr_assign.hip) and its numpy statement awr_amd.track.assign_step: numpy only.

The camera is paras = (1, 1, 0, 0), flip = +1, and every coordinate is a small integer, so xyz = (u d, v d, d), every squared distance and
every gate edge are exactly representable.  `chain` draws a sequence of steps for B frames of K latent hands that walk, hide, reappear and
sometimes jump; `reference_step` is an independent restatement of one step -- plain Python floats, itertools.permutations, sets and
dicts -- that the statement is checked against on the host and the kernel, through the statement, on the device."""
import itertools
import math

import numpy as np

PARAS, FLIP = (1.0, 1.0, 0.0, 0.0), 1
OK, EMPTY, BAD_WINDOW = 0, 1, 3
NAMES = ("centers", "status", "code", "reset", "source", "dropped")
STATE = ("last_uvd", "ids", "miss", "next_id")
CFG = dict(gate_mm=6.0, merge_mm=2.0, max_miss=2)


def same(a, b):
    """np.array_equal with NaN positions equal"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def chain(K, B, T=12, seed=0, tracked=False):
    """-> T steps (cand_uvd (K, B, 3) float64, cand_status (K, B) int32, trk_uvd, trk_status or None, None).  Per frame K latent hands on an
    integer grid: a step moves u and v by -1 ... 1, rarely the depth (a jump in x = u d: out of the gate); a hand hides for 1 ... 4 steps
    now and then.  The visible hands come in random candidate order; unused candidate rows are EMPTY with NaN, and now and then a row is OK
    with a NaN or an infinite coordinate, or finite with a status that is not OK.  A tracked row shows a random latent hand's position --
    two slots may show the same one -- and is OK with probability 0.6."""
    rs = np.random.RandomState(1000 * K + 10 * B + seed)
    pos = np.stack([rs.randint(0, 30, (B, K)), rs.randint(0, 30, (B, K)), rs.randint(1, 4, (B, K))], -1).astype(np.float64)      # (B, K, 3)
    hidden = np.zeros((B, K), np.int64)
    steps = []
    for _ in range(T):
        pos[..., :2] += rs.randint(-1, 2, (B, K, 2))
        jump = rs.uniform(size=(B, K)) < 0.05
        pos[..., 2] = np.where(jump, rs.randint(1, 4, (B, K)), pos[..., 2])
        hidden = np.where(hidden > 0, hidden - 1, np.where(rs.uniform(size=(B, K)) < 0.15, rs.randint(1, 5, (B, K)), 0))
        cand, cstat = np.full((K, B, 3), np.nan), np.full((K, B), EMPTY, np.int32)
        for b in range(B):
            seen = [h for h in rs.permutation(K) if hidden[b, h] == 0]
            for j, h in enumerate(seen):
                cand[j, b], cstat[j, b] = pos[b, h], OK
                roll = rs.uniform()
                if roll < 0.04:
                    cand[j, b, rs.randint(3)] = (np.nan, np.inf, -np.inf)[rs.randint(3)]
                elif roll < 0.08:
                    cstat[j, b] = (EMPTY, BAD_WINDOW)[rs.randint(2)]
        trk = tstat = None
        if tracked:
            which = rs.randint(0, K, (K, B))
            trk = np.ascontiguousarray(np.stack([pos[np.arange(B), which[k]] for k in range(K)]))
            tstat = np.where(rs.uniform(size=(K, B)) < 0.6, OK, EMPTY).astype(np.int32)
            trk[rs.uniform(size=(K, B)) < 0.03] = np.nan
        steps.append((cand, cstat, trk, tstat))
    return steps


def _xyz(c):
    u, v, d = (float(x) for x in c)
    return ((u - PARAS[2]) * d / PARAS[0], (v - PARAS[3]) * d / PARAS[1] * float(FLIP), d)


def _d2(a, b):
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return (dx * dx + dy * dy) + dz * dz


def _finite(c):
    return all(math.isfinite(float(x)) for x in c)


def reference_step(state, cand, cstat, trk=None, tstat=None, cfg=CFG, n_valid=None):
    """One step, restated independently of awr_amd.track.assign_step.  state: dict of last_uvd, ids, miss, next_id (numpy, updated in place).
    -> dict of centers, status, code, reset, source, dropped.  The codes are spelt as numbers on purpose (include/awr_hip.h AWR_ASSIGN_*)."""
    K, B = state["ids"].shape
    nv = B if n_valid is None else n_valid
    gate2, merge2, max_miss = float(cfg["gate_mm"]) ** 2, float(cfg["merge_mm"]) ** 2, cfg["max_miss"]
    out = dict(centers=np.full((K, B, 3), np.nan), status=np.full((K, B), EMPTY, np.int32), code=np.zeros((K, B), np.int32),
               reset=np.zeros((K, B), np.int32), source=np.full((K, B), -1, np.int32), dropped=np.zeros(B, np.int32))
    for b in range(nv):
        live = {i for i in range(K) if state["ids"][i, b] > 0}
        held = {i for i in live if trk is not None and tstat[i, b] == OK and _finite(trk[i, b])}
        where = {i: _xyz(trk[i, b]) if i in held else _xyz(state["last_uvd"][i, b]) for i in live}
        gone = {}                                                  # slot -> code of a released identity
        for i, j in itertools.combinations(range(K), 2):
            if i in held and j in held and _d2(where[i], where[j]) <= merge2:
                young = max((i, j), key=lambda s: state["ids"][s, b])
                gone[young] = 6
                held.discard(young)
                live.discard(young)
        usable = [j for j in range(K) if cstat[j, b] == OK and _finite(cand[j, b])]
        cost = {(i, j): _d2(where[i], _xyz(cand[j, b])) for i in live for j in usable}
        ok_pairs = {ij for ij, c in cost.items() if c <= gate2}
        best = None
        for perm in itertools.permutations(range(K)):
            pairs = [(i, perm[i]) for i in range(K) if (i, perm[i]) in ok_pairs]
            total = 0.0
            for ij in pairs:
                total = total + cost[ij]
            key = (-len(pairs), total)
            if best is None or key < best[0]:
                best = (key, dict(pairs))
        match = best[1]
        taken = set(match.values())
        centre, code = {}, {}
        for i in sorted(live):
            if i in held:
                centre[i], code[i], state["miss"][i, b] = ("t", i), 3, 0
            elif i in match:
                centre[i], code[i], state["miss"][i, b] = ("c", match[i]), 2, 0
            else:
                state["miss"][i, b] += 1
                if state["miss"][i, b] <= max_miss:
                    code[i] = 4
                else:
                    gone[i] = 5
        for i, c in gone.items():
            live.discard(i)
            code[i] = c
            state["ids"][i, b], state["miss"][i, b], state["last_uvd"][i, b] = 0, 0, np.nan
        for j in usable:
            if j in taken:
                continue
            free = [i for i in range(K) if i not in live]
            coasting = [i for i in live if code[i] == 4]
            if free:
                slot = free[0]
            elif coasting:
                slot = min(coasting, key=lambda s: (-state["miss"][s, b], s))
            else:
                out["dropped"][b] += 1
                continue
            live.add(slot)
            centre[slot], code[slot] = ("c", j), 1
            state["ids"][slot, b], state["miss"][slot, b] = state["next_id"][b], 0
            state["next_id"][b] += 1
            out["reset"][slot, b] = 1
        for i in range(K):
            out["code"][i, b] = code.get(i, 0)
            if i in centre and code[i] in (1, 2, 3):
                kind, j = centre[i]
                out["centers"][i, b] = trk[i, b] if kind == "t" else cand[j, b]
                out["status"][i, b], out["source"][i, b] = OK, -2 if kind == "t" else j
                state["last_uvd"][i, b] = out["centers"][i, b]
    return out


def new_state(T, K, B):
    return dict(zip(STATE, T.identity_state(K, B)))


def copy_state(state):
    return {k: v.copy() for k, v in state.items()}


def run(T, state, cand, cstat, trk=None, tstat=None, cfg=CFG, n_valid=None, **kw):
    """assign_step on a state dict -> dict of its six outputs"""
    got = T.assign_step(state["last_uvd"], state["ids"], state["miss"], state["next_id"], cand, cstat, trk, tstat, cfg, n_valid, PARAS, FLIP, **kw)
    return dict(zip(NAMES, got))


def frame(K, rows, status=None):
    """one frame's K candidate (or tracked) rows: `rows` a list of (u, v, d) or None -> ((K, 1, 3) float64, (K, 1) int32)"""
    c, s = np.full((K, 1, 3), np.nan), np.full((K, 1), EMPTY, np.int32)
    for j, r in enumerate(rows):
        if r is not None:
            c[j, 0], s[j, 0] = r, OK
    if status is not None:
        s[:len(status), 0] = status
    return c, s

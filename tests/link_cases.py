"""Cases for awr_detect_hands_link (csrc/awr_hands.hip) and its numpy statements awr_amd.detect.components / hand_seeds
with `edge`, `link` and `gap`: numpy only, fixed seeds.  A case is a frame, the detector's knobs and the three link knobs; `flood_linked` is
the literal reference the statement is held to -- an explicit edge list from a per-pixel walk, then a plain breadth-first search: a
different algorithm from the statement's shifted arrays and runs.  References are computed once per (case, knobs) for K = MAX_HANDS and
shared, read-only, as tests/edge_cases.py does."""
import collections
import functools

import numpy as np

import edge_cases as EC
import hands_cases as HC

SMALL = EC.SMALL                                 # 33 x 130 and 48 x 64: the sizes that cross the 64 x 16 tiles with remainders
TRIPLES = ((0, 0, 1), (12.5, 12.5, 8), (40, 40, 32), (40, float("inf"), 64))          # (edge, link, gap) every frame of hands_cases runs at
GPU_TRIPLES = (TRIPLES[1], TRIPLES[3])           # ... and the two of them the GPU test runs
REAR, FRONT = 850, 700
OVER_LINK, OVER_GAP = 40, 32                     # the composites of edge_cases.overlap_host(): edge = 40, min_pixels = 400


def flood_linked(frame, depth_range=(1.0, 2000.0), reach=300.0, edge=None, link=None, gap=32):
    """-> labels (fh, fw) int32, the smallest raster index of the pixel's component, -1 off the mask.  The edge list: every mask pixel
    with each 4-neighbour in the mask whose raw depth, as float64, differs by at most `edge` (None: no test); and, with a link, every
    mask pixel p with the pixel q its walk in each of the four directions ends at -- over n consecutive occluders (d != 0 and
    d_p - d > edge), 1 <= n <= gap, to the first pixel that is none, inside the frame -- when q is in the mask and |d_q - d_p| <= link.
    Then a breadth-first search from every unlabelled mask pixel in raster order."""
    zmin, zmax = float(depth_range[0]), float(depth_range[1])
    fh, fw = frame.shape
    out = np.full((fh, fw), -1, np.int32)
    fg = (frame >= zmin) & (frame <= zmax) & (frame != 0)
    if not fg.any():
        return out
    mask = fg & (frame <= min(float(frame[fg].min()) + float(reach), zmax))
    d = frame.astype(np.float64).tolist()
    inmask = mask.tolist()
    adj = collections.defaultdict(list)

    def inside(v, u):
        return 0 <= v < fh and 0 <= u < fw

    for v, u in zip(*(x.tolist() for x in np.nonzero(mask))):
        dp = d[v][u]
        for dv, du in ((0, 1), (0, -1), (1, 0), (-1, 0)):
            nv, nu = v + dv, u + du
            if inside(nv, nu) and inmask[nv][nu] and (edge is None or abs(dp - d[nv][nu]) <= edge):
                adj[(v, u)].append((nv, nu))
                adj[(nv, nu)].append((v, u))
            if link is None:
                continue
            n = 0                                                   # the consecutive occluders q_1 ... q_n, counted up to gap
            while n < gap and inside(v + (n + 1) * dv, u + (n + 1) * du):
                o = d[v + (n + 1) * dv][u + (n + 1) * du]
                if not (o != 0 and dp - o > edge):
                    break
                n += 1
            qv, qu = v + (n + 1) * dv, u + (n + 1) * du
            if n == 0 or not inside(qv, qu):                        # p does not walk, or the walk leaves the frame
                continue
            dq = d[qv][qu]
            if dq != 0 and dp - dq > edge:                          # q_1 ... q_gap and q_{gap + 1} are all occluders
                continue
            if inmask[qv][qu] and abs(dq - dp) <= link:
                adj[(v, u)].append((qv, qu))
                adj[(qv, qu)].append((v, u))
    for v0, u0 in zip(*(x.tolist() for x in np.nonzero(mask))):
        if out[v0, u0] >= 0:
            continue
        root = v0 * fw + u0
        out[v0, u0] = root
        todo = collections.deque([(v0, u0)])
        while todo:
            p = todo.popleft()
            for q in adj.get(p, ()):
                if out[q] < 0:
                    out[q] = root
                    todo.append(q)
    return out


def center(shape):
    """the point the occlusions cross: row 16, and column 64 where the frame has one"""
    return 16, 64 if shape[1] > 64 else 32


def crossed(shape, vertical=False, thick=4, rear=REAR, front=FRONT, rear2=None):
    """edge_cases.occlusion: a rear rectangle crossed by a nearer bar `thick` pixels thick, horizontal (through row 16) or vertical
    (through column 64 / 32).  rear2: the depth of the rectangle's second half (below / right of the bar)"""
    cv, cu = center(shape)
    rear2 = rear if rear2 is None else rear2
    if not vertical:
        f = EC.occlusion(shape, cv, cu, rear, front)
        f[cv + 2:cv + 10, cu - 14:cu + 16] = rear2
        f[cv - 2:cv + 2, cu - 24:cu + 30] = 0
        f[cv - 2:cv - 2 + thick, cu - 24:cu + 30] = front
        if thick < 4:
            f[cv - 2 + thick:cv + 2, cu - 14:cu + 16] = rear2
        return f
    f = np.zeros(shape, np.uint16)
    f[max(cv - 14, 0):cv + 16, cu - 8:cu - 2] = rear
    f[max(cv - 14, 0):cv + 16, cu - 2 + thick:max(cu + 10, cu - 2 + thick + 6)] = rear2
    f[max(cv - 24, 0):cv + 30, cu - 2:cu - 2 + thick] = front
    return f


def chain(shape):
    """three rear pieces A, B, C in a row with a bar between each two; C starts two rows higher, so the chain's smallest index is C's
    and A and B reach it only through links.  The bars are taller than the pieces: no path leads round them"""
    f = np.zeros(shape, np.uint16)
    f[10:21, 10:20], f[10:21, 24:34], f[8:21, 38:48] = REAR, REAR + 10, REAR + 20
    f[6:25, 20:24], f[6:25, 34:38] = FRONT, FRONT + 5
    return f


def wide_bar(shape, width):
    """two rear pieces with a bar of `width` columns between them, rows 10 ... 20"""
    f = np.zeros(shape, np.uint16)
    f[10:21, 20:33], f[10:21, 33 + width:33 + width + 13], f[8:23, 33:33 + width] = REAR, REAR, FRONT
    assert 33 + width + 13 <= shape[1]
    return f


def border_ring(shape):
    """the frame at the rear depth with a ring of 4 nearer pixels round it: every walk leaves the frame"""
    f = np.full(shape, FRONT, np.uint16)
    f[4:-4, 4:-4] = REAR
    return f


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(name, frame (read-only), depth_range, reach, slab, min_pixels, edge, link, gap)"""
    out = {}
    add = lambda name, frame, **k: HC._add(out, name, frame, **dict(dict(edge=40, link=40, gap=32, min_pixels=20), **k))      # noqa: E731
    for shape in SMALL:
        tag = "%dx%d_" % shape
        cv, cu = center(shape)
        for way, vertical in (("h", False), ("v", True)):
            add(tag + "gap4_joins_" + way, crossed(shape, vertical), gap=4)
            add(tag + "gap3_splits_" + way, crossed(shape, vertical), gap=3)
            for link in (40, 12.5, 0):
                k = int(np.floor(link))
                add(tag + "agree_exact_%s_l%g" % (way, link), crossed(shape, vertical, rear2=REAR + k), link=link)
                add(tag + "agree_plus1_%s_l%g" % (way, link), crossed(shape, vertical, rear2=REAR + k + 1), link=link)
        for edge in (40, 12.5):
            e = int(np.floor(edge))
            add(tag + "occluder_plus1_e%g" % edge, crossed(shape, front=REAR - e - 1), edge=edge)
            add(tag + "occluder_exact_e%g" % edge, crossed(shape, front=REAR - e), edge=edge)
        f = crossed(shape)
        f[cv - 1, cu - 24:cu + 30] = REAR + 100                      # a row of the bar FARTHER than the rectangle: it ends every walk
        add(tag + "farther_between", f)
        f = crossed(shape, rear=850, front=800, rear2=830)           # only the 850 half sees an occluder; the 830 half joins the bar
        add(tag + "one_sided", f)
        f = crossed(shape)
        f[cv - 1, cu] = 0                                            # a zero pixel in the bar: that column's walks end on it
        add(tag + "zero_hole", f)
        f = np.zeros(shape, np.uint16)
        f[cv - 8:cv + 10, cu], f[cv - 2:cv + 2, cu - 3:cu + 4] = REAR, FRONT
        add(tag + "one_column", f, min_pixels=1)
        f = f.copy()
        f[cv - 1, cu] = 0
        add(tag + "one_column_zero_hole", f, min_pixels=1)
        add(tag + "border_ring", border_ring(shape), gap=4)
        add(tag + "border_ring_gap64", border_ring(shape), gap=64)
        add(tag + "bar_nearer_than_zmin", crossed(shape), depth_range=(750.0, 2000.0))
        add(tag + "half_beyond_reach", crossed(shape, rear2=FRONT + 301), link=float("inf"))
        add(tag + "half_at_reach", crossed(shape, rear2=FRONT + 300), link=float("inf"))
        add(tag + "chain", chain(shape))
        add(tag + "chain_gap3", chain(shape), gap=3)
        add(tag + "fragments_below_min_pixels", crossed(shape), min_pixels=300)
        frame, edge = EC.smooth_field(shape, 11 + shape[0])
        for gap in (1, 5, 64):
            add(tag + "smooth_field_gap%d" % gap, frame, edge=edge, link=2 * edge, gap=gap, min_pixels=6)
    shape = SMALL[0]
    add("33x130_bar64_gap64", wide_bar(shape, 64), gap=64)
    add("33x130_bar64_gap63", wide_bar(shape, 64), gap=63)
    add("33x130_bar65_gap64", wide_bar(shape, 65), gap=64)
    return out


LINK_KNOBS = ("edge", "link", "gap")


def knobs(c):
    return dict(HC.knobs(c), **{k: c[k] for k in LINK_KNOBS})


def groups(which=None):
    """(shape, knobs with the link's) -> the names of the cases that share them, in a fixed order"""
    out = {}
    for name, c in (cases() if which is None else which).items():
        out.setdefault((c["frame"].shape,) + tuple(knobs(c).values()), []).append(name)
    return out


def _statement(frame, K, k):
    import awr_amd  # noqa: F401
    from awr_amd import detect as D
    labels = D.components(frame, k["depth_range"], k["reach"], k["edge"], k["link"], k["gap"])
    centers, status, info, count = D.hand_seeds(frame, K, **k)
    for a in (labels, centers, status, info):
        a.setflags(write=False)
    return labels, centers, status, info, count


@functools.lru_cache(maxsize=None)
def reference(name, triple=None):
    """-> (labels, centres (4, 3), status (4,), info (4, 4), count) of the statement, read-only.  name: a case of this file (its own
    knobs), or one of hands_cases' cases at triple = (edge, link, gap)"""
    if name in cases():
        c = cases()[name]
        return _statement(c["frame"], 4, knobs(c))
    c = HC.cases()[name]
    return _statement(c["frame"], 4, dict(HC.knobs(c), edge=triple[0], link=triple[1], gap=triple[2]))


@functools.lru_cache(maxsize=None)
def overlap_reference(i, link=OVER_LINK, gap=OVER_GAP):
    """the statement on composite i of edge_cases.overlap_host(), edge = 40, min_pixels = 400 -> as reference(); link None: edge alone"""
    frame = EC.overlap_host()[2][i]
    return _statement(frame, 4, dict(HC.knobs(HC.DEFAULT), min_pixels=EC.OVER_MIN_PIXELS, edge=EC.OVER_EDGE, link=link, gap=gap))


def stripes(shape=HC.FULL, gap=32, rear=REAR, front=FRONT):
    """the constructed worst case: vertical stripes of ONE rear column to `gap` front columns over the whole frame -- every rear pixel
    walks the full gap to the right and to the left"""
    f = np.full(shape, front, np.uint16)
    f[:, ::gap + 1] = rear
    return f


def n_components(labels):
    return int(np.unique(labels[labels >= 0]).size)

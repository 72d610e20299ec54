"""Cases for awr_frames_denoise (csrc/awr_denoise.hip) and its numpy statement awr_amd.detect.denoise: numpy only, fixed
seeds.  `loop` is the per-pixel Python loop the statement is held to -- the rule read off line by line, sets and a sort per pixel.  A case
is a frame; `grid` is the options every case runs at.  References are computed once per (case, options) and shared, read-only."""
import functools
import itertools

import numpy as np

NEAR = 700
TINY = [(1, 1), (1, 7), (5, 3)]               # smaller than the window
ODD = [(17, 67)]                              # an odd width: the scalar form, rows that start unaligned
TILES = [(33, 130), (48, 64)]                 # row 16 and column 64 are tile borders (48 x 64: fw a multiple of 4, the 8-byte form)
SIZES = TINY + ODD + TILES
FULL = (480, 640)
EDGES = (None, 0, 12.5, 40, float("inf"))
SUPPORTS = {1: (0, 1, 3, 8), 2: (0, 1, 3, 8, 24)}
FILLS = {1: (None, 1, 6, 8), 2: (None, 1, 6, 8, 24)}


def loop(frame, radius=1, edge=None, support=0, fill=None):
    """The rule, pixel by pixel."""
    fh, fw = frame.shape
    elim = 65535 if edge is None else int(np.floor(min(float(edge), 65535.0)))
    out = np.zeros((fh, fw), np.uint16)
    f = frame.astype(np.int64).tolist()
    for v in range(fh):
        for u in range(fw):
            dp = f[v][u]
            W = [f[y][x] for y in range(max(v - radius, 0), min(v + radius, fh - 1) + 1)
                 for x in range(max(u - radius, 0), min(u + radius, fw - 1) + 1) if (y, x) != (v, u)]
            if dp != 0:
                S = [d for d in W if d != 0 and abs(d - dp) <= elim]
                if len(S) >= support:
                    out[v, u] = sorted(S + [dp])[len(S) // 2]
            else:
                V = [d for d in W if d != 0]
                if fill is not None and len(V) >= fill:
                    out[v, u] = sorted(V)[(len(V) - 1) // 2]
    return out


def grid(radius, thin=False):
    """every (edge, support, fill) of the issue's grid at `radius`; thin: a diagonal through it that still holds every value once"""
    es, ss, fs = EDGES, SUPPORTS[radius], FILLS[radius]
    if not thin:
        return [dict(radius=radius, edge=e, support=s, fill=f) for e, s, f in itertools.product(es, ss, fs)]
    n = max(len(es), len(ss), len(fs))
    return [dict(radius=radius, edge=es[i % len(es)], support=ss[i % len(ss)], fill=fs[(i + 1) % len(fs)]) for i in range(n)]


def opt_id(o):
    return "r%d_e%s_s%d_f%s" % (o["radius"], o["edge"], o["support"], o["fill"])


# ---- the frames ------------------------------------------------------------------------------------------------------------------------
def step(shape, axis, at, gap):
    f = np.full(shape, NEAR, np.uint16)
    if axis == 0:
        f[at:] = NEAR + gap
    else:
        f[:, at:] = NEAR + gap
    return f


def _spots(shape, v, u, radius):
    return [(y, x) for y in range(v - radius, v + radius + 1) for x in range(u - radius, u + radius + 1)
            if (y, x) != (v, u) and 0 <= y < shape[0] and 0 <= x < shape[1]]


def sites(shape):
    """where a hole or a speckle is placed: the interior of a tile, two frame corners, and the corner of four tiles (or, in a frame of one
    tile row, a tile's last row); far enough apart that no window holds two of them"""
    h, w = shape
    return [(7, 9), (0, 0), (h - 1, w - 1), (16 if h > 22 else 8, 64 if w > 70 else w // 2)]


def holes(shape, valid, radius):
    """a zero frame with a hole at every site, each with exactly min(valid, the neighbours it has in the frame) valid neighbours inside its
    radius-`radius` window (the first ones in raster order, all different)"""
    f = np.zeros(shape, np.uint16)
    for v, u in sites(shape):
        for i, (y, x) in enumerate(_spots(shape, v, u, radius)[:valid]):
            f[y, x] = NEAR + 3 * i
    return f


def speckles(shape, similar, radius):
    """a surface at NEAR + 100 with a pixel at NEAR at every site that has exactly min(similar, ...) neighbours within 40 mm of it"""
    f = np.full(shape, NEAR + 100, np.uint16)
    for v, u in sites(shape):
        f[v, u] = NEAR
        for i, (y, x) in enumerate(_spots(shape, v, u, radius)[:similar]):
            f[y, x] = NEAR + 1 + i
    return f


def checker_holes(shape):
    h, w = shape
    d = NEAR + (np.add.outer(np.arange(h), 2 * np.arange(w)) % 37)
    return np.where((np.add.outer(np.arange(h), np.arange(w)) % 2) == 0, d, 0).astype(np.uint16)


def extremes(shape):
    """values 1 and 65535 side by side, in stripes two columns wide"""
    w = shape[1]
    return np.broadcast_to(np.where((np.arange(w) // 2) % 2 == 0, 1, 65535).astype(np.uint16), shape).copy()


def two_surfaces(shape):
    """2 x 2 blocks, six pixels apart on a zero frame, a row at NEAR above a row at NEAR + 30: every block pixel's window (either radius) holds
    exactly its block -- four values, two on each surface -- so with an edge of 30 or more the lower median of that EVEN count is NEAR, the
    nearer surface, on all four pixels (an upper median or an average would give NEAR + 30 or NEAR + 15)"""
    h, w = shape
    f = np.zeros(shape, np.uint16)
    for v in range(1, h - 1, 6):
        for u in range(1, w - 1, 6):
            f[v, u:u + 2], f[v + 1, u:u + 2] = NEAR, NEAR + 30
    return f


def upsampled_noise(shape, seed):
    h, w = shape
    low = np.random.RandomState(seed).randint(0, 120, (h // 4 + 1, w // 4 + 1))
    return (NEAR + np.kron(low, np.ones((4, 4), np.int64))[:h, :w]).astype(np.uint16)


def random_zeros(shape, seed, span=60):
    r = np.random.RandomState(seed)
    f = NEAR + r.randint(0, span, shape)
    f[r.uniform(size=shape) < 0.3] = 0
    return f.astype(np.uint16)


OWN = {}          # name -> the options of a case that is built around ONE threshold; every other case runs at options_for(its shape)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> frame (read-only), grouped by shape in `groups`"""
    out = {}

    def add(name, frame):
        frame = np.ascontiguousarray(frame, dtype=np.uint16)
        frame.setflags(write=False)
        assert name not in out
        out[name] = frame
    for h, w in SIZES:
        tag = "%dx%d_" % (h, w)
        shape = (h, w)
        add(tag + "zeros", np.zeros(shape, np.uint16))
        add(tag + "all_65535", np.full(shape, 65535, np.uint16))
        add(tag + "constant", np.full(shape, NEAR, np.uint16))
        add(tag + "extremes", extremes(shape))
        add(tag + "checker_holes", checker_holes(shape))
        add(tag + "random_zeros", random_zeros(shape, 3 + h))
        add(tag + "random_wide", random_zeros(shape, 5 + w, span=60000))
        if shape in TINY:
            continue
        add(tag + "two_surfaces", two_surfaces(shape))
        add(tag + "upsampled_noise", upsampled_noise(shape, 7 + h))
        borders = [("inside_row", 0, 5), ("inside_col", 1, 20)] + ([("row16", 0, 16)] if h > 16 else []) + ([("col64", 1, 64)] if w > 64 else [])
        for where, axis, at in borders:
            for edge in (40, 12.5, 0):
                e = int(np.floor(edge))
                for kind, gap in (("exact", e), ("plus1", e + 1)):
                    name = tag + "step_%s_%s_e%g" % (kind, where, edge)
                    add(name, step(shape, axis, at, gap))
                    OWN[name] = [dict(radius=r, edge=edge, support=k, fill=None) for r, k in ((1, 0), (1, 6), (2, 0), (2, 15))]
        # holes with exactly fill and fill - 1 valid neighbours, speckles with exactly support and support - 1 similar ones: each frame
        # runs at the options that make its count the threshold (OWN), with and without an edge
        for r, k in ((1, 1), (1, 6), (1, 8), (2, 6), (2, 8), (2, 24)):
            for n in (k, k - 1):
                name = tag + "holes_r%d_fill%d_n%d" % (r, k, n)
                add(name, holes(shape, n, r))
                OWN[name] = [dict(radius=r, edge=e, support=0, fill=k) for e in (None, 0)]
        for r, k in ((1, 1), (1, 3), (1, 8), (2, 3), (2, 8), (2, 24)):
            for n in (k, k - 1):
                name = tag + "speckles_r%d_support%d_n%d" % (r, k, n)
                add(name, speckles(shape, n, r))
                OWN[name] = [dict(radius=r, edge=40, support=k, fill=None), dict(radius=r, edge=39.5, support=k, fill=1)]
    return out


@functools.lru_cache(maxsize=None)
def groups():
    """shape -> the names of its cases, in a fixed order"""
    out = {}
    for name, frame in cases().items():
        out.setdefault(frame.shape, []).append(name)
    return out


def options_for(name, full=False):
    """the options a case runs at against the loop: its own where it is built around a threshold, else the grid -- all of it where the
    frame is small, thinned where it is large (the loop is Python per pixel).  full: the whole grid as well, whatever the size."""
    shape = cases()[name].shape
    thin = shape[0] * shape[1] > 600 and not full
    own = OWN.get(name)
    if own is not None and not full:
        return own
    return (own or []) + grid(1, thin) + grid(2, thin)


@functools.lru_cache(maxsize=None)
def reference(name, radius, edge, support, fill):
    """loop() on a case, once; read-only"""
    out = loop(cases()[name], radius, edge, support, fill)
    out.setflags(write=False)
    return out


# ---- 480 x 640: two noisy hands ------------------------------------------------------------------------------------------------------
NOISE_MM, N_FULL = 6, 2
FULL_OPTIONS = (dict(radius=1, edge=40, support=0, fill=None), dict(radius=2, edge=40, support=6, fill=18))


def noisy_hands():
    """-> (prims_a, bbox_a, prims_b, bbox_b) of the first N_FULL near-hand composites of tests/isolate_cases.py"""
    import isolate_cases as IC
    return tuple(x[:N_FULL] for x in IC.near_hands()[:4])


@functools.lru_cache(maxsize=None)
def noisy_host():
    """the N_FULL composites with noise_mm = NOISE_MM by the numpy renderer: (N_FULL, 480, 640) uint16, read-only"""
    from awr_amd import synth as SY
    pa, ba, pb, bb = noisy_hands()
    both = SY.compose(SY.render(pa, ba, noise_mm=NOISE_MM, seed=1), SY.render(pb, bb, noise_mm=NOISE_MM, seed=2))
    both.setflags(write=False)
    return both

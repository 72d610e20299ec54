"""Cases for awr_background_learn and awr_frames_foreground (csrc/awr_background.hip) and their numpy statements
awr_amd.background.learn and foreground: numpy only, fixed seeds.  `loop_foreground` and `loop_learn` are the per-pixel Python loops the
statements are held to -- the rules read off line by line.  An apply case is a (frame, model) pair; a learning case a stack of frames.
References are computed once and shared, read-only.  `scene` is the cluttered 480 x 640 scene of the predictor tests."""
import functools

import numpy as np

SHAPES = [(48, 64), (37, 53), (16, 8)]          # 48 x 64 and 16 x 8: the 16-byte form; 37 x 53: the scalar form, a ragged last thread
FULL = (480, 640)
MARGINS = (0, 30.0, 12.7, 65535, float("inf"))
UNKNOWNS = ("keep", "drop")
STEPS = (None, 1, 7, 65535)
RANK_NAMES = ("min", "median", "max")
LEARN_N = (1, 2, 3, 63, 64)


def loop_foreground(frame, model, margin=30.0, unknown="keep", adapt=None):
    """The apply rule, pixel by pixel: -> (out, new_model)"""
    fh, fw = frame.shape
    mg = int(np.floor(min(float(margin), 65535.0)))
    out, new = np.zeros((fh, fw), np.uint16), np.array(model, np.uint16)
    f, mm = frame.astype(np.int64).tolist(), model.astype(np.int64).tolist()
    for v in range(fh):
        for u in range(fw):
            d, m = f[v][u], mm[v][u]
            if m == 0:
                keep = d != 0 and unknown == "keep"
            else:
                keep = d != 0 and d + mg < m
            out[v, u] = d if keep else 0
            if adapt is not None and d != 0 and m != 0 and not keep:
                new[v, u] = m + min(max(d - m, -adapt), adapt)
    return out, new


def loop_learn(frames, rank="median", min_valid=1):
    """The learning rule, pixel by pixel"""
    n, fh, fw = frames.shape
    out = np.zeros((fh, fw), np.uint16)
    f = frames.astype(np.int64).tolist()
    for v in range(fh):
        for u in range(fw):
            V = sorted(f[i][v][u] for i in range(n) if f[i][v][u] != 0)
            if len(V) >= min_valid:
                out[v, u] = V[{"min": 0, "median": (len(V) - 1) // 2, "max": len(V) - 1}[rank]]
    return out


def options(thin=False):
    """every (margin, unknown, adapt); thin: a diagonal that still holds every value once"""
    if not thin:
        return [dict(margin=m, unknown=u, adapt=s) for m in MARGINS for u in UNKNOWNS for s in STEPS]
    n = max(len(MARGINS), len(STEPS))
    return [dict(margin=MARGINS[i % len(MARGINS)], unknown=UNKNOWNS[i % 2], adapt=STEPS[(i + 1) % len(STEPS)]) for i in range(n)]


def opt_id(o):
    return "m%s_%s_a%s" % (o["margin"], o["unknown"], o["adapt"])


def _pair(shape, seed, span=200):
    """a model with unknown pixels and a frame around it: zeros, pixels on either side of the model and exactly at the margins' edges"""
    r = np.random.RandomState(seed)
    m = 800 + r.randint(0, span, shape)
    m[r.uniform(size=shape) < 0.2] = 0
    d = m + r.randint(-60, 20, shape)
    at = r.uniform(size=shape)
    d = np.where(at < 0.15, 0, np.where(at < 0.3, m - 30, np.where(at < 0.4, m - 31, np.where(at < 0.5, m - 12, np.where(at < 0.55, m - 13, d)))))
    d = np.where(m == 0, 700 + r.randint(0, 300, shape), d)
    d[r.uniform(size=shape) < 0.1] = 0
    return np.clip(d, 0, 65535).astype(np.uint16), m.astype(np.uint16)


def _wide(shape, seed):
    r = np.random.RandomState(seed)
    d, m = r.randint(0, 65536, shape), r.randint(0, 65536, shape)
    d[r.uniform(size=shape) < 0.1] = 0
    m[r.uniform(size=shape) < 0.1] = 0
    return d.astype(np.uint16), m.astype(np.uint16)


@functools.lru_cache(maxsize=None)
def apply_cases():
    """name -> (frame, model), read-only"""
    out = {}

    def add(name, d, m):
        d, m = np.ascontiguousarray(d, dtype=np.uint16), np.ascontiguousarray(m, dtype=np.uint16)
        d.setflags(write=False)
        m.setflags(write=False)
        out[name] = (d, m)
    for i, shape in enumerate(SHAPES):
        tag = "%dx%d_" % shape
        add(tag + "around", *_pair(shape, 3 + i))
        add(tag + "wide", *_wide(shape, 13 + i))
        add(tag + "no_model", _pair(shape, 23 + i)[0], np.zeros(shape))
        add(tag + "all_65535", np.full(shape, 65535), np.full(shape, 65535))
        add(tag + "zero_frame", np.zeros(shape), _pair(shape, 33 + i)[1])
        # the last pixels of the frame differ from everything else: a ragged last thread that reads or writes one pixel too many shows
        d, m = np.full(shape, 500), np.full(shape, 900)
        d.reshape(-1)[-5:] = (0, 900, 869, 870, 1)
        m.reshape(-1)[-3:] = (0, 871, 2)
        add(tag + "tail", d, m)
    return out


@functools.lru_cache(maxsize=None)
def apply_groups():
    out = {}
    for name, (d, _) in apply_cases().items():
        out.setdefault(d.shape, []).append(name)
    return out


@functools.lru_cache(maxsize=None)
def apply_reference(name, margin, unknown, adapt):
    """the STATEMENT on a case, once; read-only (tests/test_background_cpu.py holds the statement to the loop)"""
    import awr_amd  # noqa: F401
    from awr_amd import background as BG
    out, new = BG.foreground(*apply_cases()[name], margin=margin, unknown=unknown, adapt=adapt)
    out.setflags(write=False)
    new.setflags(write=False)
    return out, new


@functools.lru_cache(maxsize=None)
def learn_frames(shape, n, seed=0):
    """n frames of a noisy surface with holes: pixels valid in every frame, in none, in few; ties (a pixel's depths take few values); a
    pixel column valid in exactly 0 ... n frames along the first row"""
    r = np.random.RandomState(100 + seed + n + shape[1])
    f = 900 + r.randint(0, 6, (n,) + shape)                              # few values: ties
    f[:, 2:] += r.randint(0, 3000, (n,) + (shape[0] - 2, shape[1]))[:, :]          # ... and a wide spread below the first two rows
    f[r.uniform(size=f.shape) < 0.35] = 0
    f[:, :, 1] = 0                                                         # valid in no frame
    f[:, :, 2] = 1200 + np.arange(n)[:, None]                              # valid in every frame, all different
    for u in range(min(shape[1] - 3, n + 1)):                             # row 0, column 3 + u: valid in exactly u frames
        f[:, 0, 3 + u] = np.where(np.arange(n) < u, 65535 - np.arange(n), 0)
    f = np.ascontiguousarray(np.clip(f, 0, 65535), dtype=np.uint16)
    f.setflags(write=False)
    return f


def learn_options(n):
    mv = sorted({1, 2, (n + 1) // 2, n} & set(range(1, n + 1)))
    return [dict(rank=r, min_valid=k) for r in RANK_NAMES for k in mv]


@functools.lru_cache(maxsize=None)
def learn_reference(shape, n, rank, min_valid, zeroed=()):
    """the STATEMENT on learn_frames(shape, n), frames `zeroed` replaced by zeros (a listed index outside the store), once; read-only"""
    import awr_amd  # noqa: F401
    from awr_amd import background as BG
    f = np.array(learn_frames(shape, n))
    for i in zeroed:
        f[i] = 0
    out = BG.learn(f, rank, min_valid)
    out.setflags(write=False)
    return out


# ---- 480 x 640: hands in front of static clutter ---------------------------------------------------------------------------------------
WALL_MM, BAR_MM, CLUTTER_NOISE_MM, N_EMPTY, N_SCENE = 1500, 450, 4, 5, 3


def clutter_prims():
    """a bar across the lower frame BAR_MM from the camera -- nearer than every hand -- and a body-sized capsule at 1000 mm to the left"""
    import awr_amd  # noqa: F401
    from awr_amd import nyu_data as ND
    y = -(440.0 - ND.PARAS[3]) * BAR_MM / ND.PARAS[1]
    prims = np.zeros((1, 2, 8))
    prims[0, 0] = (-400.0, y, BAR_MM, 400.0, y, BAR_MM, 25.0, 0.0)
    prims[0, 1] = (-380.0, 150.0, 1000.0, -380.0, -400.0, 1000.0, 120.0, 0.0)
    return prims


@functools.lru_cache(maxsize=None)
def scene():
    """-> a namespace, every array read-only: empty (N_EMPTY, 480, 640) hand-free frames of the clutter in front of a wall with
    CLUTTER_NOISE_MM of noise; model, their lower median; hands (N_SCENE, 480, 640) the clutter-free near-hand frames of
    tests/isolate_cases.py; frames, each composed with a noisy clutter frame of its own (what the sensor gives); masked,
    background.foreground(frames[i], model) at the defaults"""
    import types
    import awr_amd  # noqa: F401
    from awr_amd import background as BG
    from awr_amd import synth as SY
    import isolate_cases as IC
    n = N_EMPTY + N_SCENE
    box = np.array([[0, 0, FULL[1], FULL[0]]] * n, np.int32)
    clutter = SY.render(np.repeat(clutter_prims(), n, 0), box, background_mm=WALL_MM, noise_mm=CLUTTER_NOISE_MM, seed=11)
    empty = clutter[:N_EMPTY]
    model = BG.learn(empty)
    hands = np.array(IC.near_hands_host()[2][:N_SCENE])
    frames = SY.compose(hands, clutter[N_EMPTY:])
    masked = np.stack([BG.foreground(f, model)[0] for f in frames])
    out = types.SimpleNamespace(empty=empty, model=model, hands=hands, frames=frames, masked=masked)
    for a in vars(out).values():
        a.setflags(write=False)
    return out

"""The f64 reference of the demo-proximity reward (robot.py:749-757) and of the exact two-level
nearest-demo index (include/navenv.h, csrc/demo_index.hip), restated in plain numpy from their
definitions, and the ragged layout the CPU and GPU tests share. Imports no torch and no library:
the index resolution R (nav_demo_index_res()) is an argument.

Every value is formed by the same IEEE f64 operations in the same order as the kernels form it
(the library is built with -ffp-contract=off; numpy's elementwise ops do not fuse), so the tests
compare for equality, not within a tolerance.

  min2(points, s)        min_j (dx*dx + dy*dy) over the whole set
  reward(gt, m2, stuck)  gt + demo_factor * (-sqrt(m2)), then - stuck_penalty
  level1 / level2        bound, count, start and the candidate lists of index cells
"""
import os

import numpy as np

WORLD = 100             # dynamics cells per side (NAV_WORLD_CELLS)
L1_CELLS = WORLD * WORLD
DEMO_FACTOR = 10.0      # robot.py:43
STUCK_PENALTY = 50.0    # robot.py:41
F_STUCK, F_DEMO = 4, 16  # nav_step_out.flags bits 2 and 4
_BUDGET = 1 << 21       # elements of one vectorised chunk


# ---------------------------------------------------------------- reward
def sqd(points, s):
    """[k][m] squared distances dx*dx + dy*dy of k states to m points."""
    points = np.asarray(points, np.float64).reshape(-1, 2)
    s = np.asarray(s, np.float64).reshape(-1, 2)
    dx = s[:, None, 0] - points[None, :, 0]
    dy = s[:, None, 1] - points[None, :, 1]
    return dx * dx + dy * dy


def min2(points, s):
    """min_j (dx*dx + dy*dy) of each state of s [k][2] (or [2]) over all points [m][2]; +inf for
    an empty set. A minimum does not depend on the order it is taken in."""
    points = np.asarray(points, np.float64).reshape(-1, 2)
    s2 = np.asarray(s, np.float64).reshape(-1, 2)
    out = np.full(len(s2), np.inf)
    step = max(1, _BUDGET // max(1, len(points)))
    for i in range(0, len(s2), step):
        if len(points):
            out[i:i + step] = sqd(points, s2[i:i + step]).min(1)
    return out[0] if np.ndim(s) == 1 else out


def argmin2(points, s):
    """first index of the nearest point of each state (ties: the lowest index)"""
    s2 = np.asarray(s, np.float64).reshape(-1, 2)
    step = max(1, _BUDGET // max(1, len(points)))
    return np.concatenate([sqd(points, s2[i:i + step]).argmin(1)
                           for i in range(0, len(s2), step)])


def reward(gt, m2, stuck, demo_factor=DEMO_FACTOR, stuck_penalty=STUCK_PENALTY):
    """demo_reward_of's operation order: gt + demo_factor * (-sqrt(min2)), then - stuck_penalty
    where stuck."""
    gt = np.asarray(gt, np.float64)
    r = gt + demo_factor * (-np.sqrt(np.asarray(m2, np.float64)))
    return np.where(np.asarray(stuck, bool), r - stuck_penalty, r)


def wave_sum32(v):
    """The wave's f32 xor-tree sum (offsets 32, 16, .. 1) of 64 lane values, lane 0's result: the
    reward column of a block_stats row."""
    v = np.asarray(v, np.float32).copy()
    assert v.shape == (64,)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return v[0]


# ---------------------------------------------------------------- the index
def in_index(s):
    s = np.asarray(s, np.float64).reshape(-1, 2)
    return (s[:, 0] >= 0.0) & (s[:, 0] < 100.0) & (s[:, 1] >= 0.0) & (s[:, 1] < 100.0)


def index_cell(s, res):
    """index cell ((int)(x*R)) * 100R + (int)(y*R) of states inside the index"""
    s = np.asarray(s, np.float64).reshape(-1, 2)
    side = WORLD * res
    return (s[:, 0] * res).astype(np.int64) * side + (s[:, 1] * res).astype(np.int64)


def parent_of(cells, res):
    """dynamics cell cx*100 + cy of index cells"""
    side = WORLD * res
    cells = np.asarray(cells, np.int64)
    return (cells // side // res) * WORLD + (cells % side) // res


def cell_maxd2(px, py, lx, ly, w):
    """squared distance of a point to the farthest point of the cell [lx, lx+w] x [ly, ly+w]"""
    fx = np.maximum(np.abs(px - lx), np.abs(px - (lx + w)))
    fy = np.maximum(np.abs(py - ly), np.abs(py - (ly + w)))
    return fx * fx + fy * fy


def cell_mind2(px, py, lx, ly, w):
    """squared distance of a point to the nearest point of the cell"""
    nx = np.maximum(0.0, np.maximum(lx - px, px - (lx + w)))
    ny = np.maximum(0.0, np.maximum(ly - py, py - (ly + w)))
    return nx * nx + ny * ny


def limit_of(u2):
    """the candidate test's bound from U^2 = min_q maxdist^2(q, cell)"""
    return u2 * (1.0 + 1e-12) + 1e-12


class Level:
    """One level's result on `cells` (ascending cell ids): bound f64, count i32, start i64
    (exclusive scan over these cells, total last) and cand (the lists, concatenated)."""

    def __init__(self, cells, bound, lists):
        self.cells = np.asarray(cells, np.int64)
        self.bound = bound
        self.count = np.array([len(x) for x in lists], np.int32)
        self.start = np.zeros(len(lists) + 1, np.int64)
        self.start[1:] = np.cumsum(self.count, dtype=np.int64)
        self.cand = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
        self._slot = {int(c): i for i, c in enumerate(self.cells)}

    def slot(self, cell):
        return self._slot[int(cell)]

    def list_of(self, cell):
        i = self._slot[int(cell)]
        return self.cand[self.start[i]:self.start[i + 1]]


def level1(points, cells=None):
    """Level 1 over all of a group's points: per dynamics cell (cx*100 + cy, w = 1) the bound
    lim(U^2), and the ascending indices of the points with mindist^2 <= bound."""
    points = np.asarray(points, np.float64).reshape(-1, 2)
    cells = np.arange(L1_CELLS) if cells is None else np.unique(np.asarray(cells, np.int64))
    px, py = points[None, :, 0], points[None, :, 1]
    bound = np.zeros(len(cells))
    lists = []
    step = max(1, _BUDGET // len(points))
    for i in range(0, len(cells), step):
        c = cells[i:i + step]
        lx = (c // WORLD).astype(np.float64)[:, None]
        ly = (c % WORLD).astype(np.float64)[:, None]
        lim = limit_of(cell_maxd2(px, py, lx, ly, 1.0).min(1))
        take = cell_mind2(px, py, lx, ly, 1.0) <= lim[:, None]
        bound[i:i + step] = lim
        lists += [np.nonzero(t)[0] for t in take]
    return Level(cells, bound, lists)


def level2(points, l1, res, cells=None):
    """Level 2: per index cell (ix*100R + iy, w = 1/R, low corner cx + sx*w) the bound from its
    level-1 parent's list alone, and the parent's entries, in the parent's order, with
    mindist^2 <= bound. `l1` must hold the parents of `cells`."""
    points = np.asarray(points, np.float64).reshape(-1, 2)
    side = WORLD * res
    cells = np.arange(side * side) if cells is None else np.unique(np.asarray(cells, np.int64))
    w = 1.0 / res
    par = np.array([l1.slot(c) for c in parent_of(cells, res)], np.int64)
    plen = l1.count[par].astype(np.int64)
    order = np.argsort(plen, kind="stable")  # chunks of similar parent length: little padding
    bound = np.zeros(len(cells))
    lists = [None] * len(cells)
    i = 0
    while i < len(order):
        sel = order[i:i + 4096]
        sel = sel[:max(1, _BUDGET // int(plen[sel[-1]]))]  # plen ascends: the last is the longest
        i += len(sel)
        L = int(plen[sel[-1]])
        col = np.arange(L)[None, :]
        valid = col < plen[sel][:, None]
        at = np.where(valid, l1.start[par[sel]][:, None] + col, 0)
        idx = l1.cand[at]
        px, py = points[idx, 0], points[idx, 1]
        ix, iy = cells[sel] // side, cells[sel] % side
        lx = ((ix // res).astype(np.float64) + (ix % res).astype(np.float64) * w)[:, None]
        ly = ((iy // res).astype(np.float64) + (iy % res).astype(np.float64) * w)[:, None]
        u2 = np.where(valid, cell_maxd2(px, py, lx, ly, w), np.inf).min(1)
        lim = limit_of(u2)
        take = valid & (cell_mind2(px, py, lx, ly, w) <= lim[:, None])
        bound[sel] = lim
        for r, c in enumerate(sel):
            lists[c] = idx[r][take[r]]
    return Level(cells, bound, lists)


def build(points, res, cells=None):
    """(level 1 on the parents of `cells`, level 2 on `cells`); every cell when cells is None"""
    l1 = level1(points, None if cells is None else parent_of(cells, res))
    return l1, level2(points, l1, res, cells)


def gather(start, cand, cells):
    """(count, start-relative lists concatenated) of `cells` from a device-layout (start, cand)
    pair of one group: what Level.count / Level.cand hold for the same cells."""
    a, b = start[cells], start[np.asarray(cells) + 1]
    cnt = (b - a).astype(np.int64)
    rel = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return cnt.astype(np.int32), cand[np.repeat(a, cnt) + rel]


# ---------------------------------------------------------------- the shared ragged layout
EPG = 96    # envs per group: 64-env waves sit inside one group and straddle two
N_ENVS = 470  # 5 groups, the last one partial; not a multiple of 64; workgroup 0 spans A, B, C
GROUPS = "ABCDE"
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trace.npz")


def ragged_layout():
    """(points [m][2], off [6]) of five demo sets of unequal size:
    A 1 point; B 3 collinear points, two of them identical (ties); C 70 points on integer and
    quarter-integer cell edges and corners, 16 of them outside the world on every side; D the
    golden trace's 11 355-point set; E 17 identical points (every list: 17 = 16 + 1 = 2*8 + 1)."""
    rng = np.random.default_rng(20240611)
    a = np.array([[37.3, 61.8]])
    b = np.array([[20.0, 30.0], [20.0, 30.0], [60.0, 30.0]])
    c = [rng.integers(0, 101, (18, 2)).astype(np.float64),          # dynamics-cell corners
         rng.integers(0, 401, (18, 2)) / 4.0]                       # index-cell corners
    e1 = rng.uniform(0, 100, (18, 2))                               # on one cell edge
    e1[:9, 0] = rng.integers(0, 101, 9)
    e1[9:, 1] = rng.integers(0, 401, 9) / 4.0
    c.append(e1)
    t = rng.uniform(0, 100, 16)
    c.append(np.array([[-0.5, t[0]], [-3.25, t[1]], [-40.0, 50.0], [-1e-9, t[3]],
                       [100.0, t[4]], [100.25, t[5]], [104.5, t[6]], [260.0, 10.0],
                       [t[8], -0.25], [t[9], -7.0], [30.0, -55.0], [t[11], -1e-9],
                       [t[12], 100.0], [t[13], 101.0], [99.75, 180.0], [-2.0, 103.0]]))
    c = np.concatenate(c)
    d = np.load(_GOLDEN)["demo_set"].astype(np.float64)
    e = np.tile(np.array([[55.125, 44.6]]), (17, 1))
    sets = [a, b, c, d, e]
    assert [len(x) for x in sets] == [1, 3, 70, 11355, 17]
    off = np.zeros(6, np.int64)
    off[1:] = np.cumsum([len(x) for x in sets])
    return np.ascontiguousarray(np.concatenate(sets)), off


RING_N = 180           # envs of the ring layout: 96 of group 0, 84 of group 1
RING_CENTRE = (50.3, 49.9)


def ring_layout():
    """(points, off [3]) of a layout with long lists: group 0 is 300 points on a circle of radius
    20, all of them candidates of every cell near its centre (the ragged layout's longest list
    has 28 entries); group 1 is 17 identical points."""
    th = 2.0 * np.pi * np.arange(300) / 300.0
    ring = np.stack([RING_CENTRE[0] + 20.0 * np.cos(th), RING_CENTRE[1] + 20.0 * np.sin(th)], 1)
    same = np.tile(np.array([[12.5, 80.25]]), (17, 1))
    return np.ascontiguousarray(np.concatenate([ring, same])), np.array([0, 300, 317], np.int64)


def ring_states(seed=12):
    """[RING_N][2]: two thirds of group 0's envs within 0.15 of the circle's centre (lists of
    about 300), the rest of the states uniform in the world"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0, 100, (RING_N, 2))
    e = np.arange(RING_N)
    close = (e < EPG) & (e % 3 != 0)
    s[close] = np.array(RING_CENTRE) + rng.uniform(-0.15, 0.15, (int(close.sum()), 2))
    return s


def group_of(e, epg=EPG):
    return np.asarray(e) // epg


def query_states(points, off, res, n=N_ENVS, epg=EPG, seed=11):
    """[n][2] query states, per group in equal shares (env e of the group takes kind e % 6):
    uniform in the world; dynamics-cell corners; index-cell corners; the group's demo points
    inside the world; within +-0.4 of them; the borders 0 and nextafter(100, 0). Group B's
    uniform share lies on x = 40, equidistant from its two distinct points."""
    rng = np.random.default_rng(seed)
    top = np.nextafter(100.0, 0.0)
    s = rng.uniform(0, 100, (n, 2))
    for e in range(n):
        g = e // epg
        pts = points[off[g]:off[g + 1]]
        inside = pts[in_index(pts)]
        kind = (e % epg) % 6
        if kind == 0 and g == 1:
            s[e, 0] = 40.0
        elif kind == 1:
            s[e] = np.floor(s[e])
        elif kind == 2:
            s[e] = np.floor(s[e] * res) / res
        elif kind == 3:
            s[e] = inside[rng.integers(0, len(inside))]
        elif kind == 4:
            s[e] = inside[rng.integers(0, len(inside))] + rng.uniform(-0.4, 0.4, 2)
            s[e] = np.clip(s[e], 0.0, top)
        elif kind == 5:
            edge = np.array([0.0, top])
            which = rng.integers(0, 3)
            if which != 1:
                s[e, 0] = edge[rng.integers(0, 2)]
            if which != 0:
                s[e, 1] = edge[rng.integers(0, 2)]
    assert in_index(s).all()
    return s


def cell_probes(cell, res, rng, n_random=4):
    """query states inside index cell `cell`: its low corner, the low edges' midpoints, the
    centre, the last representable states before the high edges, and random interior points"""
    side = WORLD * res
    w = 1.0 / res
    lx, ly = (cell // side) * w, (cell % side) * w
    hx, hy = np.nextafter(lx + w, 0.0), np.nextafter(ly + w, 0.0)
    mx, my = lx + 0.5 * w, ly + 0.5 * w
    fixed = [(lx, ly), (lx, hy), (hx, ly), (hx, hy), (mx, ly), (mx, hy), (lx, my), (hx, my),
             (mx, my)]
    rnd = np.stack([rng.uniform(lx, lx + w, n_random), rng.uniform(ly, ly + w, n_random)], 1)
    s = np.concatenate([np.array(fixed), np.clip(rnd, [lx, ly], [hx, hy])])
    assert (index_cell(s, res) == cell).all()
    return s

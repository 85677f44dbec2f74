"""What makes demo_ref.py trustworthy, without a GPU: on the ragged layout its level-2 lists hold
the brute-force nearest point of every query inside their cell, the minimum over a list is the
minimum over the whole group bit for bit, and the lists are strictly ascending indices into the
group, each a subset of its level-1 parent's list."""
import numpy as np
import pytest

import demo_ref as D


@pytest.fixture(scope="module")
def res():
    from nav import _lib
    return int(_lib.lib().nav_demo_index_res())


@pytest.fixture(scope="module")
def layout(res):
    pts, off = D.ragged_layout()
    return pts, off, D.query_states(pts, off, res)


def cells_checked(g, layout, res, n_random):
    """index cells of group g to check: the cells its query states fall in, the grid's four
    corner cells, the cells of its own points inside the world, and n_random random ones"""
    pts, off, s = layout
    side = D.WORLD * res
    rng = np.random.default_rng(100 + g)
    mine = s[D.group_of(np.arange(len(s))) == g]
    own = pts[off[g]:off[g + 1]]
    own = own[D.in_index(own)][:200]
    return np.unique(np.concatenate([
        D.index_cell(mine, res), D.index_cell(own, res),
        np.array([0, side - 1, side * (side - 1), side * side - 1]),
        rng.integers(0, side * side, n_random)]))


def test_layout_is_ragged(layout):
    pts, off, s = layout
    assert list(np.diff(off)) == [1, 3, 70, 11355, 17]
    assert len(s) == D.N_ENVS == 470 and D.N_ENVS % 64 != 0 and D.EPG % 64 != 0
    g = D.group_of(np.arange(D.N_ENVS))
    assert g.max() == 4 and (g == 4).sum() == 86              # the last group is partial
    waves = [np.unique(g[w:w + 64]) for w in range(0, D.N_ENVS, 64)]
    assert any(len(w) == 1 for w in waves) and any(len(w) == 2 for w in waves)
    assert len(np.unique(g[:256])) == 3                        # one workgroup, three groups
    c = pts[off[2]:off[3]]
    assert (c[:, 0] < 0).any() and (c[:, 0] >= 100).any()
    assert (c[:, 1] < 0).any() and (c[:, 1] >= 100).any()
    assert (c[:54] * 4 == np.round(c[:54] * 4)).any(1).all()  # on quarter-integer lines
    b = pts[off[1]:off[2]]
    assert np.array_equal(b[0], b[1]) and b[0, 1] == b[2, 1]
    assert (np.diff(pts[off[4]:off[5]], axis=0) == 0).all()


@pytest.mark.parametrize("g,n_random", [(0, 1500), (1, 1500), (2, 1500), (3, 400), (4, 1500)])
def test_lists_hold_the_nearest_point_of_every_probe(layout, res, g, n_random):
    pts, off, _ = layout
    P = pts[off[g]:off[g + 1]]
    cells = cells_checked(g, layout, res, n_random)
    l1, l2 = D.build(P, res, cells)
    assert np.array_equal(l2.cells, cells)
    rng = np.random.default_rng(7 + g)
    probes = np.concatenate([D.cell_probes(c, res, rng) for c in cells])
    per = len(probes) // len(cells)
    whole = D.min2(P, probes)
    near = D.argmin2(P, probes)
    assert np.isfinite(whole).all()
    longest = 0
    for i, c in enumerate(cells):
        lst = l2.list_of(c)
        parent = l1.list_of(D.parent_of(c, res))
        # strictly ascending, inside [0, m_g), a subset of the parent's list
        assert len(lst) >= 1 and lst[0] >= 0 and lst[-1] < len(P), (g, c)
        assert (np.diff(lst) > 0).all() and (np.diff(parent) > 0).all(), (g, c)
        assert np.isin(lst, parent).all(), (g, c)
        q = slice(i * per, (i + 1) * per)
        assert np.isin(near[q], lst).all(), (g, c)
        assert np.array_equal(D.min2(P[lst], probes[q]), whole[q]), (g, c)
        longest = max(longest, len(lst))
    if g == 4:
        assert (l2.count == 17).all()   # 16 + 1 = 2 * 8 + 1 in every cell
    if g == 3:
        assert longest > 8              # lists of more than one trip (the set's longest: 28)
    if g == 0:
        assert (l2.count == 1).all()


def test_level2_is_level1_restricted(layout, res):
    """A subcell's list taken from its parent's list equals the list taken from all of the
    group's points with the subcell's own bound: the parent restriction drops no candidate."""
    pts, off, _ = layout
    P = pts[off[2]:off[3]]
    cells = cells_checked(2, layout, res, 800)
    _, l2 = D.build(P, res, cells)
    side = D.WORLD * res
    w = 1.0 / res
    for c in cells:
        ix, iy = c // side, c % side
        lx, ly = (ix // res) + (ix % res) * w, (iy // res) + (iy % res) * w
        lim = D.limit_of(D.cell_maxd2(P[:, 0], P[:, 1], lx, ly, w).min())
        full = np.nonzero(D.cell_mind2(P[:, 0], P[:, 1], lx, ly, w) <= lim)[0]
        assert np.isin(full, l2.list_of(c)).all(), c
        assert l2.bound[l2.slot(c)] >= lim


def test_same_candidate_sets_as_the_cpu_port(layout, res, orc):
    """The CPU port's index (oracle/nav_oracle.c, written apart from the kernels' and from
    demo_ref) lists the same points per cell, in its own order: group C on every cell, group D
    on the checked sample."""
    pts, off, _ = layout
    P = pts[off[2]:off[3]]
    _, l2 = D.build(P, res)
    ix = orc.DemoIndexCPU(P)
    assert ix.total == l2.start[-1]
    assert np.array_equal(ix.start, l2.start)
    owner = np.repeat(np.arange(len(l2.count)), l2.count)
    theirs = ix.cand[:ix.total][np.lexsort((ix.cand[:ix.total], owner))]
    assert np.array_equal(theirs, l2.cand)
    P = pts[off[3]:off[4]]
    cells = cells_checked(3, layout, res, 2000)
    _, l2 = D.build(P, res, cells)
    ix = orc.DemoIndexCPU(P)
    count, theirs = D.gather(ix.start, ix.cand, cells)
    assert np.array_equal(count, l2.count)
    owner = np.repeat(np.arange(len(cells)), count)
    assert np.array_equal(theirs[np.lexsort((theirs, owner))], l2.cand)


def test_reward_and_wave_sum_order():
    r = D.reward(np.array([-3.0, -3.0]), np.array([4.0, 4.0]), np.array([False, True]))
    assert r[0] == -3.0 + 10.0 * -2.0 and r[1] == r[0] - 50.0
    assert D.reward(-1.0, np.inf, False) == -np.inf
    v = np.random.default_rng(0).standard_normal(64).astype(np.float32)
    t = v.copy()
    for o in (32, 16, 8, 4, 2, 1):
        t = np.array([t[i] + t[i ^ o] for i in range(64)], np.float32)
    assert D.wave_sum32(v) == t[0]
    assert D.min2(np.zeros((0, 2)), np.array([1.0, 2.0])) == np.inf

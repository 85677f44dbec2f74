"""Multi-step returns restated on the host (include/navenv.h, nav_nstep_*): Python floats for the
double sum and the powers of gamma, np.float32 for the final roundings, oracle.philox for the
indices the row kernels draw themselves. Needs no GPU and no libnavenv.so."""
import numpy as np

from oracle import oracle as O

NAV_TAG_SAMPLE = 4
NSTEP_MAX = 16
# why a horizon ended where it did (rows(..., causes=[])), the first that holds in the header's
# order: n_step rows summed, the cut mark of a row that is not `done`, the cut mark of a `done`
# row, the ring's write head
CAUSES = ("n_step", "cut", "done", "head")


def draw(size, B, seed, counter):
    """idx [B] int64: (w.x * size) >> 32 of Philox NAV_TAG_SAMPLE at ctr = (b, 0, 4, 2*counter),
    the critic row kernels' own draw."""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    c3 = (2 * int(counter)) & 0xFFFFFFFF
    return np.array([(int(O.philox((b, 0, NAV_TAG_SAMPLE, c3), key)[0]) * int(size)) >> 32
                     for b in range(B)], np.int64)


def rows(ring, cut, size, position, stride, n_step, gamma_f32, idx, causes=None):
    """(staged [B][8] float32, steps [B] int32) of nav_nstep_rows for the ring indices `idx`,
    following the header comment literally. `causes` (a list, optional) receives one of CAUSES
    per row."""
    ring = np.asarray(ring, np.float32)
    cap = ring.shape[0]
    assert ring.shape == (cap, 8) and len(cut) == cap and 1 <= size <= cap
    assert 0 <= position < cap and (size == cap or position == size)
    assert stride >= 1 and 1 <= n_step <= NSTEP_MAX
    g = float(np.float32(gamma_f32))
    idx = np.asarray(idx, np.int64)
    staged = np.empty((len(idx), 8), np.float32)
    steps = np.empty(len(idx), np.int32)
    for b, k0 in enumerate(idx.tolist()):
        assert 0 <= k0 < size
        age = (position - 1 - k0) % cap  # rows written after k0
        k = lambda j: (k0 + j * stride) % cap  # noqa: E731
        m = 1
        while not (m == n_step or cut[k(m - 1)] != 0 or m * stride > age):
            m += 1
        R, gp = float(ring[k0, 4]), 1.0
        for j in range(1, m):
            gp = gp * g
            R = R + gp * float(ring[k(j), 4])
        last = ring[k(m - 1)]
        staged[b, :4] = ring[k0, :4]
        staged[b, 4] = np.float32(R)
        staged[b, 5:7] = last[5:7]
        staged[b, 7] = np.float32(1.0) if last[7] != 0 else np.float32(1.0 - gp)
        steps[b] = m
        if causes is not None:
            if m == n_step:
                causes.append("n_step")
            elif cut[k(m - 1)] != 0:
                causes.append("done" if last[7] != 0 else "cut")
            else:
                causes.append("head")
    return staged, steps


def discount(staged, gamma_f32):
    """The discount the critic row kernels apply to min Q' of each staged row, in their f32
    operations: gamma * (1.0f - staged[7])."""
    return np.float32(gamma_f32) * (np.float32(1) - np.asarray(staged, np.float32)[:, 7])


def stamp(cut, pos, flags):
    """The cut marks after nav_nstep_stamp: cut[(pos + i) % capacity] = bit 3 of flags[i]."""
    out = np.asarray(cut, np.uint8).copy()
    flags = np.asarray(flags, np.uint8)
    cap = out.shape[0]
    assert 0 <= pos < cap and flags.shape[0] <= cap
    for i, f in enumerate(flags.tolist()):
        out[(pos + i) % cap] = (f >> 3) & 1
    return out


def random_ring(capacity, seed, cut_p=0.2, done_p=0.05):
    """A seeded ring for the kernel tests: rewards of mixed sign and magnitude with +-50 among
    them, about one row in five cut and one in twenty done (a done row is always cut, as the tick
    writes it); column 0 is the row's own index. -> (ring [capacity][8] float32, cut [capacity] uint8)."""
    rng = np.random.default_rng(seed)
    ring = rng.standard_normal((capacity, 8)).astype(np.float32)
    ring[:, 0] = np.arange(capacity)  # a staged row names the ring row it started from
    r = rng.standard_normal(capacity) * np.where(rng.random(capacity) < 0.5, 1e-3, 7.0)
    big = rng.random(capacity)
    r = np.where(big < 0.1, 50.0, np.where(big < 0.2, -50.0, r))
    ring[:, 4] = r.astype(np.float32)
    done = rng.random(capacity) < done_p
    cut = (done | (rng.random(capacity) < cut_p - done_p)).astype(np.uint8)
    ring[:, 7] = done.astype(np.float32)
    return ring, cut


# ---- the kernel tests' cases (tests/test_gpu_nstep.py; their coverage is checked on the host too)
# (capacity, size, position, stride): full and wrapped with a capacity that is no multiple of the
# stride; part full; stride == capacity (every horizon 1); a larger ring
RINGS = [(50, 50, 13, 7), (50, 33, 33, 7), (64, 64, 0, 64), (4096, 4096, 1000, 64)]
NSTEPS = [1, 2, 3, NSTEP_MAX]
BATCHES = [1, 257]  # one row; a partial last block
RING_SEED = 20


def given_idx(capacity, size, position, stride, n_step, B, seed=RING_SEED):
    """The explicit indices of one kernel case: the newest row, the oldest row,
    position - 1 - j*stride for j = 1 .. n_step (where the ring holds such a row), a row whose
    chain wraps through slot 0 (where one exists), then seeded draws; cut to B."""
    age = lambda k: (position - 1 - k) % capacity  # noqa: E731
    idx = [(position - 1) % capacity, position % capacity if size == capacity else 0]
    idx += [(position - 1 - j * stride) % capacity for j in range(1, n_step + 1)
            if j * stride <= size - 1]
    wraps = [k for k in range(max(0, capacity - stride), size) if age(k) >= stride]
    idx += wraps[-1:]
    rng = np.random.default_rng(seed + capacity + size + n_step + B)
    idx += rng.integers(0, size, max(0, B - len(idx))).tolist()
    out = np.array(idx[:B], np.int64)
    assert out.min() >= 0 and out.max() < size
    return out

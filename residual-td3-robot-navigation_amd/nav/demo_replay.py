"""The demonstrations' transitions as replay rows (robot.py:704-716), for learning from them.

The reference pushes every demonstration transition into its replay buffer and keeps the
demonstrated states and actions (robot.py:694-695). The vectorised ring of 4 * n_envs rows is
overwritten within a few steps, so here the transitions live where the ticks never write:

- frame 0, the learner's frame (s, a, r, s', done as process_demonstration pushes them, the action
  CEM's raw one): in the tail behind the replay ring (ReplayRing(tail=...)), addressed by sample
  indices >= capacity (nav_td3_mix_idx);
- frame 1, the acting frame (s - g, the residual clamp(a) - (s - g) the actor would have to output,
  s' - g): a tensor of its own, used by the behaviour-cloning pretraining (TD3.pretrain_bc).

Both come from nav_demo_transitions; `transitions_ref` is its numpy restatement.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import torch

from ._lib import lib, params_struct, ptr, stream_handle


class DemoReplay:
    def __init__(self, states, actions, goals, params=None, ring=None, stream=None):
        """states, actions [n][T][2] float32 device tensors (nav.cem.batched_demonstrations),
        goals [n][2] (each demonstration's goal, float64). With `ring` (a ReplayRing whose tail
        has n * (T - 1) rows) the frame-0 rows are written into that tail."""
        n, T = int(states.shape[0]), int(states.shape[1])
        dev = states.device
        self.n_demo, self.T, self.n_rows = n, T, n * (T - 1)
        p = params if params is not None else params_struct()
        gl = torch.as_tensor(np.ascontiguousarray(goals), dtype=torch.float64).to(dev)
        assert states.shape == actions.shape == (n, T, 2) and gl.shape == (n, 2)
        st, ac = states.contiguous().float(), actions.contiguous().float()
        if ring is not None:
            assert ring.tail.shape == (self.n_rows, 8) and ring.tail.is_contiguous()
            self.rows0 = ring.tail
        else:
            self.rows0 = torch.zeros(self.n_rows, 8, dtype=torch.float32, device=dev)
        self.rows1 = torch.zeros(self.n_rows, 8, dtype=torch.float32, device=dev)
        for frame, rows in ((0, self.rows0), (1, self.rows1)):
            lib().nav_demo_transitions(C.byref(p), n, T, ptr(st), ptr(ac), ptr(gl), frame,
                                       ptr(rows), stream_handle(stream))

    @classmethod
    def from_rows(cls, rows0, rows1, ring=None):
        """From stored rows (a checkpoint): no launch."""
        self = cls.__new__(cls)
        self.n_rows = int(rows1.shape[0])
        self.n_demo = self.T = None
        assert rows0.shape == rows1.shape == (self.n_rows, 8)
        if ring is not None:
            assert ring.tail.shape == (self.n_rows, 8)
            ring.tail.copy_(rows0.to(ring.tail.device))
            self.rows0 = ring.tail
        else:
            self.rows0 = rows0.contiguous()
        self.rows1 = rows1.to(self.rows0.device).contiguous()
        return self

    def rows(self, frame):
        return self.rows1 if frame else self.rows0


def _neg_norm(dx, dy):
    """-sqrt(fma(dy, dy, dx * dx)) as the tick forms its goal term (nav_device.h norm2), exactly:
    the fused multiply-add through rationals, rounded once."""
    sq = float(Fraction(dy) * Fraction(dy) + Fraction(dx * dx))
    return -float(np.sqrt(np.float64(sq)))


def transitions_ref(states, actions, goals, frame, goal_threshold=5.0, goal_reward=50.0,
                    max_action=5.0):
    """nav_demo_transitions on the host: states, actions [n][T][2] float32, goals [n][2] float64
    -> rows [n * (T - 1)][8] float32, bit for bit."""
    st = np.asarray(states, np.float32)
    ac = np.asarray(actions, np.float32)
    gl = np.asarray(goals, np.float64)
    n, T = st.shape[:2]
    rows = np.zeros((n * (T - 1), 8), np.float32)
    for d in range(n):
        g = gl[d]
        for i in range(T - 1):
            s, a, ns = st[d, i].astype(np.float64), ac[d, i].astype(np.float64), \
                st[d, i + 1].astype(np.float64)
            nd = ns - g
            gt = _neg_norm(float(nd[0]), float(nd[1]))
            r = goal_reward if gt >= -goal_threshold else gt
            row = rows[d * (T - 1) + i]
            if frame == 0:
                row[0:2], row[2:4], row[5:7] = st[d, i], ac[d, i], st[d, i + 1]
            else:
                sd = s - g
                row[0:2] = sd.astype(np.float32)
                row[2:4] = (np.clip(a, -max_action, max_action) - sd).astype(np.float32)
                row[5:7] = nd.astype(np.float32)
            row[4] = np.float32(r)
            row[7] = 1.0 if i == T - 2 else 0.0
    return rows

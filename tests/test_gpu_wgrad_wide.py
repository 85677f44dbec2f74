"""The factored weight-gradient kernel's 256 (n) x 32 (k) wave tile (k_wgrad_fact<8, 1, 1>, taken
when hp % 256 == 0) and the forms kept for the other widths (128 x 64 at hp 128, 64 x 64 at hp
192), d_in 4, d_out 1, 2 hidden layers throughout.

Reference: fp64 dW_1 = dz_1^T h_0 over a slab's own rows with the forward's own ReLU bits (as
test_gpu_mlp.test_weight_grads_2layer_edge_cases builds it for the sum of the slabs), bound 1e-5
of the reference's scale (the two-plane fp16 split with fp32 accumulation measures 2e-7 to 8e-7).
Per slab the scale is that slab's own max |dW|, which is no larger than the sum's."""
import pytest
import torch

from gpu_support import nav  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
D_IN, D_OUT, NH = 4, 1, 2


def make_net(hidden, seed):
    from nav.mlp import DeviceMLP
    from oracle.td3_oracle import make_mlp_params
    p = make_mlp_params(seed, [D_IN] + [hidden] * NH + [D_OUT])
    net = DeviceMLP(D_IN, D_OUT, hidden, NH, DEV).load(p)
    return net, [(torch.tensor(W), torch.tensor(b)) for W, b in p]


def relu_bits(masks, hp, hidden, M):
    """The forward's ReLU bit image ([nh][M / 32 row tiles][hp / 32][64 lanes] u16 words, C
    layout: bit i of lane (l32, h) = row (i & 3) + 8 (i >> 2) + 4 h of the tile, column l32) as
    [nh][M][hidden] booleans."""
    nt = hp // 32
    w = masks.cpu().to(torch.int32) & 0xFFFF
    n_rt = w.numel() // (NH * nt * 64)
    bits = ((w.view(NH, n_rt, nt, 2, 32, 1) >> torch.arange(16)) & 1).bool()
    r = torch.arange(32)
    hh, ii = (r >> 2) & 1, (r & 3) + 4 * (r >> 3)
    b = bits.permute(0, 1, 3, 5, 2, 4)[:, :, hh, ii]
    return b.reshape(NH, n_rt * 32, nt * 32)[:, :M, :hidden]


class Case:
    """One forward of `n` nets on the same M rows (its ReLU bits kept), their dy rows, and the
    per-row fp64 factors of dW_1."""

    def __init__(self, hidden, M, n=1, seed=0):
        from nav.mlp import forward
        self.hidden, self.M = hidden, M
        made = [make_net(hidden, 140 + M + 7 * k + seed) for k in range(n)]
        self.nets = [m[0] for m in made]
        self.layers = [m[1] for m in made]
        self.hp = self.nets[0].hp
        g = torch.Generator().manual_seed(5000 + M + seed)
        self.x = (torch.randn(M, D_IN, generator=g) * 20).contiguous()
        self.dy = [torch.randn(M, D_OUT, generator=g) / M for _ in range(n)]
        self.xd = self.x.to(DEV)
        self.dyd = [d.to(DEV).contiguous() for d in self.dy]
        self.masks = [net.mask_buffer(M) for net in self.nets]
        self.acts = torch.zeros(NH, M, self.hp, device=DEV)
        self.dz = torch.zeros(NH, M, self.hp, device=DEV)
        out = torch.zeros(M, D_OUT, device=DEV)
        for net, mk in zip(self.nets, self.masks):
            forward([net], self.xd, D_IN, 0, [out], D_OUT, 0, M, acts=[self.acts], masks=[mk])
        torch.cuda.synchronize()

    def factors(self, k):
        """(dz_1, h_0) of net k in fp64, dz_1 under the forward's own layer-1 ReLU bits."""
        W0, b0 = self.layers[k][0]
        h0 = torch.relu(torch.nn.functional.linear(self.x.double(), W0.double(), b0.double()))
        bits = relu_bits(self.masks[k], self.hp, self.hidden, self.M)
        dz1 = (self.dy[k].double() @ self.layers[k][NH][0].double()) * bits[1].double()
        return dz1, h0

    def launch(self, which, splits):
        """nav_mlp_wgrad of the nets `which` in one launch into NaN-filled slabs; returns one
        [splits][hc] tensor per net."""
        from nav._lib import descs, lib, parr, ptr, stream_handle
        L = lib()
        hc = max(4, L.nav_mlp_hidden_count(self.hp, NH))
        hs = [torch.full((splits, hc), float("nan"), device=DEV) for _ in which]
        rc = L.nav_mlp_wgrad(descs(*[self.nets[k] for k in which]), len(which), self.M,
                             ptr(self.xd), D_IN, 0, parr(*[self.acts] * len(which)),
                             parr(*[self.dz] * len(which)), parr(*[self.dyd[k] for k in which]),
                             D_OUT, parr(*[self.masks[k] for k in which]), parr(*hs), splits,
                             stream_handle())
        assert rc == 0
        torch.cuda.synchronize()
        return [h.cpu() for h in hs]


def per_split_rows(M, splits):
    return -(-(-(-M // splits)) // 32) * 32


def check_slabs(case, slabs, splits, k=0):
    """Every slab against the fp64 product over its own rows (1e-5 of that product's scale; a
    slab without rows exactly 0), padded entries exactly 0."""
    hp, hidden, M = case.hp, case.hidden, case.M
    dz1, h0 = case.factors(k)
    per = per_split_rows(M, splits)
    worst = 0.0
    for s in range(splits):
        got = slabs[s, :hp * hp].view(hp, hp).double()
        assert torch.isfinite(got).all(), s
        lo, hi = min(s * per, M), min((s + 1) * per, M)
        ref = dz1[lo:hi].t() @ h0[lo:hi]
        scale = ref.abs().max().item()
        err = (got[:hidden, :hidden] - ref).abs().max().item()
        if scale > 0:
            worst = max(worst, err / scale)
        assert err <= 1e-5 * scale, (s, err, scale)
        assert (got[hidden:, :] == 0).all() and (got[:, hidden:] == 0).all(), s
    print(f"hidden {hidden} M {M} splits {splits}: worst slab err / scale {worst:.2e}")


@pytest.mark.parametrize("M,splits", [(33, 1), (4129, 2), (2049, 7)])
def test_wide_tile_per_split_slabs(nav, M, splits):
    """hidden 256: each split's slab, not only their sum. 33 rows: one full tile in wave 0, a
    one-row tile in wave 1, six waves without rows. 4 129 rows in 2 splits:
    2 080-row splits, 288-row wave ranges, so 64 rows move from waves 4-7 to waves 0-3 (352 / 224)
    and the ragged second split (2 049 rows) ends inside wave 6. 2 049 rows in 7 splits: 320-row
    splits of 64-row wave ranges, the last split of 129 rows ending mid-tile in wave 2."""
    case = Case(256, M)
    check_slabs(case, case.launch([0], splits)[0], splits)


def test_wide_tile_padded_width(nav):
    """hidden 250 pads to hp 256, so the 256 x 32 form runs with 6 padded rows and columns: those
    entries of every slab are exactly 0, the rest within bound."""
    case = Case(250, 2049)
    assert case.hp == 256
    check_slabs(case, case.launch([0], 3)[0], 3)


def test_twins_match_single_launches_bitwise(nav):
    """Two different nets on the same rows with different dy in one launch (n_nets = 2: the twin
    critics' launch) against one launch per net at the same splits: the slabs are equal bit for
    bit, so the (net, split, tile) job decode and its XCD-grouped block order address the same
    work either way."""
    case = Case(256, 4129, n=2)
    splits = 2
    both = case.launch([0, 1], splits)
    for k in range(2):
        one = case.launch([k], splits)[0]
        assert torch.equal(both[k].view(torch.int32), one.view(torch.int32)), k
    check_slabs(case, both[1], splits, k=1)


def test_wide_tile_deterministic_and_complete(nav):
    """The same launch twice into NaN-filled slabs: bitwise-equal results and no NaN left inside
    [hp x hp] of any slab (every tile of every split written)."""
    case = Case(256, 4129)
    splits = 5
    a = case.launch([0], splits)[0]
    b = case.launch([0], splits)[0]
    hp = case.hp
    assert not torch.isnan(a[:, :hp * hp]).any()
    assert torch.equal(a[:, :hp * hp].view(torch.int32), b[:, :hp * hp].view(torch.int32))


@pytest.mark.parametrize("hidden", [128, 192])
def test_other_widths_keep_their_forms(nav, hidden):
    """hp 128 (128 x 64 tiles) and hp 192 (64 x 64 tiles) are not multiples of 256 and keep the
    two-half forms: per-split slabs within the same bound."""
    case = Case(hidden, 2049)
    assert case.hp == hidden
    check_slabs(case, case.launch([0], 7)[0], 7)

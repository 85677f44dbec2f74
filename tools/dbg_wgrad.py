"""Debug probe (not a test): nav_mlp_wgrad of a 2-hidden-layer net against fp64 at a few row
counts, printing the relative error and where the largest one sits."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "residual-td3-robot-navigation_amd"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

import torch  # noqa: E402

from mlp_ref import _f64_forward, make_net, relu_bits  # noqa: E402


def run(d_in, d_out, hidden, M, splits):
    from nav._lib import descs, lib, parr, ptr, stream_handle
    from nav.mlp import forward
    nh = 2
    net, layers = make_net(d_in, d_out, hidden, nh, 40 + M)
    hp = net.hp
    g = torch.Generator().manual_seed(3000 + M)
    x = (torch.randn(M, d_in, generator=g) * 20).contiguous()
    dy = torch.randn(M, d_out, generator=g) / max(M, 1)
    xd = x.to("cuda")
    out = torch.zeros(M, d_out, device="cuda")
    acts = torch.zeros(nh, M, hp, device="cuda")
    masks = net.mask_buffer(M)
    forward([net], xd, d_in, 0, [out], d_out, 0, M, acts=[acts], masks=[masks])
    dyd = dy.to("cuda").contiguous()
    L = lib()
    hc = max(4, L.nav_mlp_hidden_count(hp, nh))
    hs = torch.full((splits, hc), float("nan"), device="cuda")
    dz = torch.zeros(nh, M, hp, device="cuda")
    rc = L.nav_mlp_wgrad(descs(net), 1, M, ptr(xd), d_in, 0, parr(acts), parr(dz), parr(dyd),
                         d_out, parr(masks), parr(hs), splits, stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    got = hs.cpu().double().sum(0)[:hp * hp].view(hp, hp)
    bits = relu_bits(masks, nh, hp, hidden, M)
    _, zs = _f64_forward(layers, x)
    h0 = torch.relu(zs[0])
    dz1 = (dy.double() @ layers[nh][0].double()) * bits[1].double()
    ref = dz1.t() @ h0
    scale = ref.abs().max().item() + 1e-30
    e = (got[:hidden, :hidden] - ref).abs()
    i = int(e.argmax())
    n, k = divmod(i, hidden)
    ratio = (got[:hidden, :hidden] / ref.where(ref != 0, torch.ones_like(ref)))
    badk = sorted(set(int(v) for v in (e > 1e-5 * scale).nonzero()[:, 1].tolist()))[:8]
    badn = sorted(set(int(v) for v in (e > 1e-5 * scale).nonzero()[:, 0].tolist()))[:8]
    info = {"bad_k": badk, "bad_n": badn,
            "h0_at_bad_k": [float(h0[:, k].abs().max()) for k in badk],
            "h0_max": float(h0.abs().max()), "x": x[0].tolist() if M == 1 else None,
            "dy": dy[0].tolist() if M == 1 else None,
            "ratio_bad": [float(ratio[n, k]) for n in badn[:2] for k in badk[:2]]}
    return {"info": info,"d_out": d_out, "M": M, "splits": splits, "rel": e.max().item() / scale,
            "at": [n, k], "got": got[n, k].item(), "ref": ref[n, k].item(),
            "bad_frac": float((e > 1e-5 * scale).double().mean()),
            "ratio_median": float(ratio[ref.abs() > 1e-3 * scale].median())}


if __name__ == "__main__":
    for d_out in (1, 2):
        for M, splits in ((1, 1), (2049, 7)):
            print(json.dumps(run(4 if d_out == 1 else 2, d_out, 256, M, splits)), flush=True)

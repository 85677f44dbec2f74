"""Score a vectorised trainer's policy as robot-learning.py's testing mode does: one greedy test
episode per env (VecTrainer.evaluate -> nav_test_rollout, one launch), printed as one JSON line.

python tools/evaluate.py --checkpoint run.pt
python tools/evaluate.py --n-envs 4096 --hidden 256 --n-hidden 2 --seed 7 --train-steps 200
python tools/evaluate.py --n-envs 4096 --train-steps 0 --bc-pretrain 500 --bc-lr 1e-3

--bc-pretrain N first clones the demonstrations into the actor (VecTrainer.pretrain_bc: the
reference README's baseline policy by imitation) and adds the BC loss over all demonstration rows
before and after to the line; --bc-weight / --demo-fraction train with the demonstrations mixed in
(--bc-q-filter: a demonstration row is cloned only where critic 1 rates its action above the
policy's; the line gains bc_kept_fraction, the share the last policy epoch kept);
--per-alpha / --per-beta / --per-eps train with prioritised replay (not together with those two);
--n-step N trains on N-step returns (with prioritised replay or alone, not with those two);
--demo-reset-prob P starts a training episode with probability P on a state of one of its env
group's demonstrations (with any of the above; the line gains demo_reset_prob and
demo_reset_share, the episodes started that way over the envs' episode numbers).
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "residual-td3-robot-navigation_amd"))


def main():
    from nav import config as K
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoint", default=None, help="a VecTrainer.save() file")
    ap.add_argument("--n-envs", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--n-hidden", type=int, default=2)
    ap.add_argument("--batch", type=int, default=None, help="default: n_envs / 2")
    ap.add_argument("--seed", type=int, default=K.RANDOM_SEED)
    ap.add_argument("--no-demos", action="store_true")
    ap.add_argument("--train-steps", type=int, default=0)
    ap.add_argument("--max-steps", type=int, default=K.TEST_TIMEOUT * K.UPDATE_RATE)
    ap.add_argument("--episode", type=int, default=0)
    ap.add_argument("--bc-pretrain", type=int, default=0, help="BC epochs before any env step")
    ap.add_argument("--bc-lr", type=float, default=None, help="the actor's lr while pretraining")
    ap.add_argument("--bc-weight", type=float, default=0.0)
    ap.add_argument("--demo-fraction", type=float, default=0.0)
    ap.add_argument("--bc-q-filter", action="store_true",
                    help="Q-filter on the BC term (needs --bc-weight and --demo-fraction)")
    ap.add_argument("--per-alpha", type=float, default=0.0,
                    help="prioritised replay: priority exponent (0 = off)")
    ap.add_argument("--per-beta", type=float, default=0.4,
                    help="prioritised replay: importance-weight exponent")
    ap.add_argument("--per-eps", type=float, default=1e-6,
                    help="prioritised replay: added to |TD error| before the exponent")
    ap.add_argument("--n-step", type=int, default=1,
                    help="multi-step returns: the longest horizon (1 = off, at most 16)")
    ap.add_argument("--demo-reset-prob", type=float, default=0.0,
                    help="resets to demonstration states: the probability per episode (0 = off)")
    args = ap.parse_args()
    import torch
    from nav._lib import require_gpu
    from nav.trainer import VecTrainer
    require_gpu()
    if args.checkpoint:
        tr = VecTrainer.load(args.checkpoint)
    else:
        tr = VecTrainer(n_envs=args.n_envs, hidden=args.hidden, n_hidden=args.n_hidden,
                        batch=args.batch or max(args.n_envs // 2, 1), seed=args.seed,
                        envs_per_group=min(1024, args.n_envs), demos=not args.no_demos,
                        demo_reset_prob=args.demo_reset_prob,
                        # the mode fields the command line has (q_weight: the default)
                        **{k: getattr(args, k) for k in K.MODE_FIELDS if hasattr(args, k)})
    bc = {}
    if args.bc_pretrain > 0:
        bc["bc_loss_before"] = tr.bc_loss(frame=1)
        tr.pretrain_bc(args.bc_pretrain, lr=args.bc_lr)
        bc["bc_loss_after"] = tr.bc_loss(frame=1)
        bc["bc_epochs"] = args.bc_pretrain
    for _ in range(args.train_steps):
        tr.step()
    res = tr.evaluate(max_steps=args.max_steps, episode=args.episode)
    torch.cuda.synchronize()
    res["train_steps"] = tr.steps
    if tr.td3.nstep_on():
        res["n_step"] = tr.td3.cfg.n_step
    if tr.td3.cfg.bc_q_filter:
        res["bc_kept_fraction"] = tr.td3.bc_kept_fraction()
    if tr.demo_reset_prob > 0:
        res["demo_reset_prob"] = tr.demo_reset_prob
        res["demo_reset_share"] = tr.env.demo_reset_share()
    res.update(bc)
    # strict JSON: a NaN (no env reached) prints as null
    print(json.dumps({k: None if isinstance(v, float) and v != v else v for k, v in res.items()}))


if __name__ == "__main__":
    main()

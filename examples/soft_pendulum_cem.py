"""Planning on SoftPendulum-v0 by branching a resident batch: a cross-entropy-method planner over action chunks, with
`env.fork` as the branch.  The reference has one env per Python object and no way to copy its state; here env 0 is the
trajectory being controlled and envs 1..N-1 are its branches, all on one MI355X.

Each planning step:
  1. `env.fork(0, range(1, N))`   every env becomes an exact copy of env 0, on the device (one small kernel);
  2. every env executes its own chunk of `horizon` actions drawn from the planner's Gaussian (env 0: its mean) —
     one batched `env.step` per action, rewards summed on the device;
  3. the Gaussian is refit to the best tenth of the chunks (the cross-entropy step) and carried to the next step;
  4. the branch that did best becomes env 0 (`env.fork(best, 0)`): `step` has no mask, so the winning branch IS the
     trajectory's next state rather than being replayed.

    python examples/soft_pendulum_cem.py --num-envs 512 --horizon 8 --iters 20

Nothing here is tuned — it is a usage example of fork().
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gym_softrobot_amd as gsa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=512, help="env 0 plus the branches")
    ap.add_argument("--horizon", type=int, default=8, help="env.steps per planning step")
    ap.add_argument("--iters", type=int, default=20, help="planning steps")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    N, H = args.num_envs, args.horizon
    if N < 2:
        ap.error("--num-envs must be at least 2: env 0 and one branch")

    env = gsa.make_vec("SoftPendulum-v0", N, device=0)
    dev = env.backend.device
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    lo, hi = env.action_low, env.action_high
    mean = torch.zeros(H, device=dev)
    std = torch.full((H,), 0.5 * (hi - lo) / 2, device=dev)
    n_elite = max(1, (N - 1) // 10)
    branches = range(1, N)

    env.reset(seed=args.seed)
    total = 0.0
    for it in range(args.iters):
        env.fork(0, branches)
        chunks = (mean + std * torch.randn((N, H), device=dev, generator=gen)).clamp_(lo, hi)
        chunks[0] = mean
        ret = torch.zeros(N, dtype=torch.float64, device=dev)
        alive = torch.ones(N, dtype=torch.bool, device=dev)
        for t in range(H):
            _, reward, term, trunc, _ = env.step(chunks[:, t : t + 1])
            ret += torch.where(alive, reward, torch.zeros_like(reward))
            alive &= ~(term | trunc)
        elite = ret.topk(n_elite).indices
        best = int(elite[0])
        mean, std = chunks[elite].mean(0), chunks[elite].std(0, unbiased=False).clamp_min(0.05 * (hi - lo))
        if best != 0:
            env.fork(best, 0)
        total += float(ret[best])
        print(f"plan {it:3d}  best branch {best:4d}  chunk return {float(ret[best]):10.4f}  mean of batch "
              f"{float(ret.mean()):10.4f}  time {float(env.backend.state()['time'][0]):.2f}")
        if not bool(alive[best]):
            print("episode over")
            break
    print(f"return of the controlled trajectory over {it + 1} planning steps: {total:.4f}")
    env.close()


if __name__ == "__main__":
    main()

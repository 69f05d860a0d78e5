"""Exploration of SoftPendulum-v0 with an archive of visited states: restarts from a state bank, in the manner of
Go-Explore.  The reference has one env per Python object and no way to keep its state; here the archive is K slots of
the batch's state bank, on the device beside the N envs, and no env is spent on holding a state.

Each round:
  1. every env is loaded from a slot chosen on the host from the slots' recorded scores (a softmax over the return
     collected on the way to each state) — `env.load_states(slots, range(N))`, one small kernel, with
     `copy_rng=False` so that every env keeps its own random stream;
  2. all N envs roll out `--steps` env.steps with random actions, one batched `env.step` per action, rewards summed
     on the device;
  3. the best new states — score of the slot they started from plus the rollout's return — replace the archive's
     worst slots where they beat them: `env.save_states(envs, slots)`.

    python examples/soft_pendulum_restarts.py --num-envs 512 --slots 64 --rounds 20

Nothing here is tuned — it is a usage example of create_state_bank() / save_states() / load_states().
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gym_softrobot_amd as gsa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=512, help="envs that explore")
    ap.add_argument("--slots", type=int, default=64, help="states the archive holds")
    ap.add_argument("--rounds", type=int, default=20, help="load / roll out / save rounds")
    ap.add_argument("--steps", type=int, default=4, help="env.steps per rollout")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    N, K = args.num_envs, args.slots
    if N < 1 or K < 1:
        ap.error("--num-envs and --slots must be at least 1")

    env = gsa.make_vec("SoftPendulum-v0", N, device=0)
    dev = env.backend.device
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    rng = np.random.default_rng(args.seed)
    lo, hi = env.action_low, env.action_high
    env.create_state_bank(K)
    print(f"{K} slots of {env.state_bank_bytes} bytes beside {N} envs")

    env.reset(seed=args.seed)
    env.save_states([0], [0])                         # the archive starts with the reset state of env 0
    score = np.full(K, -np.inf)                       # return collected on the way to each slot's state
    score[0] = 0.0
    for it in range(args.rounds):
        held = np.nonzero(env.state_bank_filled)[0]
        w = np.exp(score[held] - score[held].max())
        start = rng.choice(held, size=N, p=w / w.sum())
        env.load_states(start, range(N), copy_rng=False)
        ret = torch.zeros(N, dtype=torch.float64, device=dev)
        alive = torch.ones(N, dtype=torch.bool, device=dev)
        for _ in range(args.steps):
            actions = lo + (hi - lo) * torch.rand((N, 1), device=dev, generator=gen)
            _, reward, term, trunc, _ = env.step(actions)
            ret += torch.where(alive, reward, torch.zeros_like(reward))
            alive &= ~(term | trunc)
        # a finished episode is no state to restart from
        reached = np.where(alive.cpu().numpy(), score[start] + ret.cpu().numpy(), -np.inf)
        best = np.argsort(-reached)[:K]               # candidates, best first
        worst = np.argsort(score)                     # slots, worst first (the empty ones at -inf lead)
        keep = [(int(e), int(k)) for e, k in zip(best, worst) if reached[e] > score[k]]
        if keep:
            envs, slots = zip(*keep)
            env.save_states(envs, slots)
            score[list(slots)] = reached[list(envs)]
        print(f"round {it:3d}  saved {len(keep):3d}  slots held {int(env.state_bank_filled.sum()):3d}  "
              f"best score {score.max():10.4f}  mean return of the rollouts {float(ret.mean()):10.4f}")
    print(f"archive after {it + 1} rounds: {int(env.state_bank_filled.sum())} states, best score {score.max():.4f}, "
          f"median {np.median(score[np.isfinite(score)]):.4f}")
    env.close()


if __name__ == "__main__":
    main()

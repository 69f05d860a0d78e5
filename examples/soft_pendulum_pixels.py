"""A rollout whose policy sees PIXELS: SoftPendulum-v0 envs resident on one MI355X, a small policy fed with
`env.render_frames()` — (N, H, W, 3) uint8 frames rendered on the device by softrod_render — and the whole
`frames -> policy -> step` chain captured once into a HIP graph with `capture_policy_step`.  Nothing leaves the GPU:
the reference renders one env at a time on the host (render_mode="rgb_array").

    python examples/soft_pendulum_pixels.py --num-envs 1024 --size 64 --steps 100

Prints frames per second (every env yields one frame per step).  The policy is random weights — this is a usage example
of render_frames(), not a training script.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gym_softrobot_amd as gsa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--size", type=int, default=64, help="frame width and height in pixels")
    ap.add_argument("--steps", type=int, default=100, help="env.steps (one episode is 125)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    N, S = args.num_envs, args.size

    env = gsa.make_vec("SoftPendulum-v0", N, device=0)
    dev = env.backend.device
    cam = env.default_camera()
    cam.width = cam.height = S
    cam.center[1] = 0.5            # the pendulum stands on the origin: frame the rod, not the pivot
    cam.half_width = 0.75

    torch.manual_seed(args.seed)
    if S % 8:
        ap.error("--size must be a multiple of 8 (the policy pools 8 x 8 blocks)")
    net = torch.nn.Sequential(                       # on 8 x 8 block means of the RGB-D frame
        torch.nn.Linear((S // 8) ** 2 * 4, 64), torch.nn.Tanh(), torch.nn.Linear(64, env.action_dim), torch.nn.Tanh(),
    ).to(dev).requires_grad_(False)
    amax = 22.0                    # the pendulum's force scale

    def policy(_obs):
        rgb, depth = env.render_frames(camera=cam, depth=True)                 # uint8 (N, S, S, 3), float32 (N, S, S)
        seen = torch.isfinite(depth)
        x = torch.cat([rgb.to(torch.float32) / 255.0, torch.where(seen, depth, torch.zeros_like(depth)).unsqueeze(-1)], dim=-1)
        pooled = x.reshape(N, S // 8, 8, S // 8, 8, 4).mean(dim=(2, 4))
        return amax * net(pooled.reshape(N, -1))

    env.reset(seed=args.seed)
    replay = env.capture_policy_step(policy)      # renders, runs the policy and steps: one graph launch per env.step
    replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    total = torch.zeros((), dtype=torch.float64, device=dev)
    for _ in range(args.steps):
        _, reward, _, _ = replay()
        total += reward.sum()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"{N} envs x {args.steps} steps at {S}x{S} RGB-D: {N * args.steps / dt:,.0f} frames/s "
          f"({1e3 * dt / args.steps:.3f} ms per step, policy and render included); mean reward {float(total) / (N * args.steps):.4f}")
    env.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Scout rollout rate on one GPU: env-steps/s of VecEnv('scout', N).rollout with uniform-random play, in the trajectory
allocation new_traj_out chooses, next to that allocation's write-probe ceiling (cs_traj_probe: the rollout's 733 B per
env-step -- 688 obs + 26 legal + 1 player + 1 action + 16 reward + 1 done -- written as zeros, no game logic). bench.py
keeps its five games; this is the tenth's measurement. The reference has no Scout rule model, so there is one policy.

  python tools/bench_scout.py [--envs 65536 262144] [--T 64] [--steps 10] [--warmup 3]
One JSON line per env count: kernel ms per launch (median and min of HIP-event times), env-steps/s from the wall time
of the timed launches, the probe's ms and the share of its rate the rollout reaches. CARDSIM_LIB picks an A/B build.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_BYTES = 688 + 26 + 1 + 1 + 16 + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, nargs='*', default=[65536, 262144])
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    import torch
    from rlcard_amd import VecEnv, _abi
    for n in args.envs:
        v = VecEnv('scout', n, seed=42, device=0)
        traj = v.new_traj_out(args.T)
        assert v.traj_bytes(args.T) == args.T * n * ROW_BYTES
        t0 = 0
        for _ in range(args.warmup):
            v.rollout(args.T, policy_seed=1, t0=t0, out=traj)
            t0 += args.T
        torch.cuda.synchronize()
        events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(args.steps)]
        w0 = time.perf_counter()
        for a, b in events:
            a.record()
            v.rollout(args.T, policy_seed=1, t0=t0, out=traj)
            b.record()
            t0 += args.T
        torch.cuda.synchronize()
        wall = time.perf_counter() - w0
        ms = [a.elapsed_time(b) for a, b in events]
        games = int(traj['done'].sum().item())
        probe = min(v.probe_traj(traj, args.T) for _ in range(3))
        med = statistics.median(ms)
        print(json.dumps({
            'game': 'scout', 'policy': 'random', 'lib': os.path.basename(_abi.LIB_PATH), 'envs': n, 'T': args.T,
            'launches': args.steps, 'kernel_ms_median': med, 'kernel_ms_min': min(ms),
            'env_steps_per_s': args.steps * args.T * n / wall, 'env_steps_per_s_kernel': args.T * n / med * 1e3,
            'bytes_per_env_step': ROW_BYTES, 'write_GBps': args.T * n * ROW_BYTES / med / 1e6,
            'write_probe_ms': probe, 'probe_over_kernel': probe / med,
            'games_finished_last_launch': games, 'steps_per_game_last_launch': args.T * n / max(games, 1),
            'placement_probe_ms': v.placement_probe_ms, 'device': torch.cuda.get_device_name(0)}), flush=True)
        del traj, v
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

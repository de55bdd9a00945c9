#!/usr/bin/env python3
"""Bridge rollout rate on one GPU: env-steps/s of VecEnv('bridge', N).rollout, in the trajectory allocation
new_traj_out chooses, next to that allocation's write-probe ceiling (cs_traj_probe: the rollout's 604 B per env-step --
573 obs + 12 legal + 1 player + 1 action + 16 reward + 1 done -- written as zeros, no game logic). bench.py keeps its
five games; this is the ninth's measurement, for uniform-random play and with BridgeDefenderNoviceRuleAgent in all four
seats (every game is then four passes and a new deal).

  python tools/bench_bridge.py [--envs 65536 262144] [--T 64] [--steps 10] [--warmup 3]
One JSON line per env count and policy: kernel ms per launch (median and min of HIP-event times), env-steps/s from the
wall time of the timed launches, the probe's ms and the share of its rate the rollout reaches.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_BYTES = 573 + 12 + 1 + 1 + 16 + 1
NOVICE = 1   # CS_POLICY_RULE_V1: BridgeDefenderNoviceRuleAgent (the reference registers no model id for it)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, nargs='*', default=[65536, 262144])
    ap.add_argument('--T', type=int, default=64)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    import torch
    from rlcard_amd import VecEnv
    for n in args.envs:
        for name, policies in (('random', None), ('novice-rule x 4', [NOVICE] * 4)):
            v = VecEnv('bridge', n, seed=42, device=0)
            traj = v.new_traj_out(args.T)
            assert v.traj_bytes(args.T) == args.T * n * ROW_BYTES
            t0 = 0
            for _ in range(args.warmup):
                v.rollout(args.T, policy_seed=1, t0=t0, out=traj, policies=policies)
                t0 += args.T
            torch.cuda.synchronize()
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                      for _ in range(args.steps)]
            w0 = time.perf_counter()
            for a, b in events:
                a.record()
                v.rollout(args.T, policy_seed=1, t0=t0, out=traj, policies=policies)
                b.record()
                t0 += args.T
            torch.cuda.synchronize()
            wall = time.perf_counter() - w0
            ms = [a.elapsed_time(b) for a, b in events]
            games = int(traj['done'].sum().item())
            probe = min(v.probe_traj(traj, args.T) for _ in range(3))
            med = statistics.median(ms)
            print(json.dumps({
                'game': 'bridge', 'policy': name, 'envs': n, 'T': args.T, 'launches': args.steps,
                'kernel_ms_median': med, 'kernel_ms_min': min(ms), 'env_steps_per_s': args.steps * args.T * n / wall,
                'env_steps_per_s_kernel': args.T * n / med * 1e3,
                'bytes_per_env_step': ROW_BYTES, 'write_GBps': args.T * n * ROW_BYTES / med / 1e6,
                'write_probe_ms': probe, 'probe_over_kernel': probe / med,
                'games_finished_last_launch': games, 'steps_per_game_last_launch': args.T * n / max(games, 1),
                'placement_probe_ms': v.placement_probe_ms, 'device': torch.cuda.get_device_name(0)}), flush=True)
            del traj, v
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

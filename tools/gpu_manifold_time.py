"""What the hull-hull contact manifold (DIYGym(..., hull_manifold_points=N)) costs: milliseconds per step with N = 1 and N = 4 on
  - the free box stack of tests/golden/box_stack.yaml at 16 384 envs (every env with a resting box-box pair),
  - ur_high_5 in bench.py's `in_contact` (every env in the crossed-forearms pose) and `mixed` (every 100th env) start states.
Eager steps bracketed by events after a warm-up, the same random actions for both N.  Prints one JSON line per case and N; also the
kernel each world selected and its contact budget.

    python tools/gpu_manifold_time.py [--steps 100] [--envs 16384]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(case, N, B):
    import torch
    import bench
    from diy_gym_amd import DIYGym
    from diy_gym_amd.scene import K
    if case == 'stack':
        env = DIYGym(os.path.join(ROOT, 'tests', 'golden', 'box_stack.yaml'), num_envs=B, device='cuda:0', seed=1, hull_manifold_points=N)
        return env, None
    env = DIYGym(os.path.join(ROOT, 'examples', 'ur_high_5', 'ur_high_5.yaml'), num_envs=B, device='cuda:0', seed=1234, hull_manifold_points=N)
    every = 1 if case == 'in_contact' else 100
    idx = torch.arange(0, B, every, device='cuda:0'); L = env.layout
    for arm in range(2):
        for j, q in enumerate(bench.CROSSED):
            o = L.link_state_off[6 * arm + j]
            env.sim.state[o + K.LS_Q, idx] = q; env.sim.state[o + K.LS_QD, idx] = 0.0; env.sim.state[o + K.LS_TARGET_POS, idx] = q
    lo, hi = bench.action_bounds(env)
    gen = torch.Generator().manual_seed(1234)
    return env, [(lo + (hi - lo) * torch.rand((B, lo.numel()), generator=gen)).to('cuda:0') for _ in range(8)]


def time_case(case, N, B, steps, warm):
    import torch
    env, ring = build(case, N, B)
    act = torch.zeros((B, max(env.layout.act_dim, 1)), device='cuda:0')
    step = lambda i: env.sim.step(env._all_slots, ring[i % 8] if ring else act)
    for i in range(warm):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        step(warm + i)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    d = env.sim.enable_diagnostics(); step(0); torch.cuda.synchronize()
    return dict(case=case, hull_manifold_points=N, envs=B, ms_per_step=round(ms, 4), kernel=env.sim.kernel_name,
                max_contacts=env.layout.max_contacts, mean_contacts=round(float(d[:, 0].float().mean()), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warm', type=int, default=60)
    ap.add_argument('--envs', type=int, default=16384)
    ap.add_argument('--cases', default='stack,in_contact,mixed')
    a = ap.parse_args()
    for case in a.cases.split(','):
        for N in (1, 4):
            print(json.dumps(time_case(case, N, a.envs, a.steps, a.warm)), flush=True)


if __name__ == '__main__':
    main()

"""bench.py --dump-outputs writes what the timed path returned after its last step, and a plain run (no --full) prints the
headline line without the extra measurements."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')
FULL_ONLY = ('roofline', 'solver', 'aged', 'api_eager', 'cpu_baseline', 'configs', 'in_contact', 'legs_seconds')


def fake_leg(B, camera=None):
    """The attributes dump_outputs reads, on CPU tensors with distinct per-env values."""
    g = torch.Generator().manual_seed(5)
    sim = SimpleNamespace(obs=torch.rand((B, 7), generator=g), rew=torch.rand((B, 2), generator=g),
                          term=(torch.rand((B, 3), generator=g) > 0.5).to(torch.uint8), rew_sum=torch.arange(B, dtype=torch.float32),
                          term_flag=(torch.arange(B) % 3 == 0).to(torch.uint8))
    cams = []
    if camera:
        w, h = camera
        cams.append(SimpleNamespace(_buffers=(torch.rand((B, w, h, 3), generator=g), torch.rand((B, w, h), generator=g),
                                              torch.randint(0, 5, (B, w, h), generator=g, dtype=torch.int32))))
    return SimpleNamespace(torch=torch, sim=sim, B=B, cameras=cams)


def test_dump_writes_every_output_as_float32(tmp_path):
    leg = fake_leg(16)
    shapes = bench.dump_outputs(leg, str(tmp_path))
    assert shapes == {'obs': [16, 7], 'reward': [16, 2], 'terminal': [16, 3], 'reward_sum': [16], 'terminal_flag': [16]}
    assert sorted(os.listdir(tmp_path)) == sorted(n + '.npy' for n in shapes)
    for name, t in (('obs', leg.sim.obs), ('reward', leg.sim.rew), ('terminal', leg.sim.term), ('reward_sum', leg.sim.rew_sum),
                    ('terminal_flag', leg.sim.term_flag)):
        a = np.load(tmp_path / (name + '.npy'))
        assert a.dtype == np.float32
        assert np.array_equal(a, t.float().numpy())


def test_dump_over_budget_keeps_a_fixed_sample_of_envs(tmp_path):
    leg = fake_leg(64, camera=(4, 5))
    per_env = 4 * (7 + 2 + 3 + 1 + 1 + 4 * 5 * 3 + 4 * 5 + 4 * 5)
    budget = 10 * per_env + 100
    a, b = tmp_path / 'a', tmp_path / 'b'
    sa = bench.dump_outputs(leg, str(a), budget=budget)
    sb = bench.dump_outputs(leg, str(b), budget=budget)
    assert sa == sb and sa['obs'] == [10, 7] and sa['camera0_rgb'] == [10, 4, 5, 3] and sa['camera0_segmentation'] == [10, 4, 5]
    assert sum(os.path.getsize(p) for p in a.iterdir()) < budget + 128 * len(sa)  # (+ the .npy headers)
    idx = np.load(a / 'env_index.npy')
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(b / 'env_index.npy'))
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 64
    assert np.array_equal(np.load(a / 'reward_sum.npy'), idx.astype(np.float32))  # rew_sum holds the env index
    for name in sa:
        assert np.array_equal(np.load(a / (name + '.npy')), np.load(b / (name + '.npy')))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / 'outputs'
    r = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--steps', '12', '--warmup', '3', '--envs-per-gpu', '128', '--dump-outputs', str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    line = json.loads(lines[0])
    for k in HEADLINE:
        assert k in line, k
    assert line['steps'] == 12 and line['warmup'] == 3 and line['ms_per_step'] > 0
    assert abs(line['value'] - 128 * 12 / (line['ms_per_step'] * 12e-3)) < 1e-6 * line['value']
    assert not [k for k in FULL_ONLY if k in line]
    obs = np.load(out / 'obs.npy')
    assert obs.dtype == np.float32 and obs.shape[0] == 128 and np.isfinite(obs).all()
    for name in ('reward', 'terminal', 'reward_sum', 'terminal_flag'):
        a = np.load(out / (name + '.npy'))
        assert a.dtype == np.float32 and a.shape[0] == 128

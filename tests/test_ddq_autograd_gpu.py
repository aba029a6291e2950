"""env.sim.forward_dynamics_fn -- calculate_forward_dynamics as a torch.autograd.Function on one forward_dynamics_derivatives launch
-- on the GPU: ur_admittance x 3 and cart_tree_fixed x 3, inputs [B, nv] and [B, 4, nv] (the first rows of tests/test_ddq_gpu.py's
pools, so the fp64 references of tests/ddq_ref.py are shared with that file).

``(f(q, qd, tau) * w).sum().backward()`` must leave ``w^T dqdd_dq``, ``w^T dqdd_dqd`` and ``w^T dqdd_dtau`` in the three ``.grad``s.  Each is
checked under the bound of ITS matrix in tests/test_ddq_gpu.py, in that matrix's measure carried through the product:
|w^T (J - J_ref)| <= |w|_1 max |J - J_ref|, so the figure is max |grad - w^T J_ref| / (|w|_1 max |J_ref|) / cond(M) per item.
"""
import numpy as np
import pytest
import torch

import test_ddq_gpu as TD
from test_fd_gpu import GROUP, dev, make

pytestmark = pytest.mark.gpu
CASES = [(scene, P) for scene in ('ur_admittance', 'cart_tree') for P in (None, 4)]


def leaves(scene, robot, B, P, grads=(True, True, True)):
    q, qd, tau = TD.points(scene, robot, B, P or 1)
    if P is None:
        q, qd, tau = q[:, 0], qd[:, 0], tau[:, 0]
    return tuple(dev(a).requires_grad_(g) for a, g in zip((q, qd, tau), grads))


@pytest.mark.parametrize('scene,P', CASES)
def test_backward_gives_the_reference_matrices_transposed_times_the_weights(scene, P, monkeypatch):
    B = 3
    env, model = make(scene, B, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n = robot.num_dofs
    _, ref = TD.reference(scene, B, P or 1, env, model)
    q, qd, tau = leaves(scene, robot, B, P)
    f = sim.forward_dynamics_fn(uid, joint_damping=True)
    qdd = f(q, qd, tau)
    assert qdd.shape == q.shape and qdd.requires_grad
    kept = sim.forward_dynamics_derivatives(uid, q.detach(), qd.detach(), tau.detach(), joint_damping=True, want=('qdd', 'dqdd_dq', 'dqdd_dqd', 'dqdd_dtau')).qdd
    assert torch.equal(qdd.detach(), kept) and qdd.data_ptr() != kept.data_ptr()   # a fresh tensor, not the backend's buffer
    w = np.random.default_rng(9).uniform(-1.0, 1.0, tuple(q.shape))
    (qdd * dev(w.astype(np.float32))).sum().backward()
    w32 = w.astype(np.float32).astype(np.float64).reshape(B, P or 1, n)
    worst = {}
    for name, leaf in (('dqdd_dq', q), ('dqdd_dqd', qd), ('dqdd_dtau', tau)):
        g = leaf.grad.cpu().numpy().astype(np.float64).reshape(B, P or 1, n)
        fig = 0.0
        for e in range(B):
            for p in range(P or 1):
                r, cond = ref[e][p]
                J = getattr(r, name)
                scale = np.abs(w32[e, p]).sum() * np.abs(J).max()
                err = np.abs(g[e, p] - w32[e, p] @ J).max()
                if np.abs(J).max() < TD.ZERO_REF:
                    assert err <= TD.ZERO_TOL * np.abs(w32[e, p]).sum()
                else:
                    fig = max(fig, err / scale / cond)
        worst[name] = fig
    print('%s x%d P=%s: %s' % (scene, B, P, ' '.join('%s %.4g' % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v < TD.BOUND[GROUP[scene]][k], (scene, k, v)


@pytest.mark.parametrize('scene,P', CASES)
def test_only_the_inputs_that_need_a_gradient_get_one_and_forward_is_one_launch(scene, P, monkeypatch):
    B = 3
    env, model = make(scene, B, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    q, qd, tau = leaves(scene, robot, B, P, (False, False, True))
    f = sim.forward_dynamics_fn(uid)
    calls = []
    entry = sim.lib.dg_world_dynamics_derivatives
    others = ('calculate_forward_dynamics', 'calculate_inverse_dynamics', 'calculate_mass_matrix')

    def counted(*args):
        calls.append('dg_world_dynamics_derivatives')
        return entry(*args)
    monkeypatch.setattr(sim.lib, 'dg_world_dynamics_derivatives', counted)
    for name in others:
        monkeypatch.setattr(sim, name, lambda *a, _n=name, **k: calls.append(_n))
    qdd = f(q, qd, tau)
    qdd.square().sum().backward()
    assert calls == ['dg_world_dynamics_derivatives']   # one launch forward, none backward
    assert q.grad is None and qd.grad is None and tau.grad is not None and tau.grad.shape == tau.shape
    Minv = sim.forward_dynamics_derivatives(uid, q, qd, tau.detach(), want=('dqdd_dtau', )).dqdd_dtau
    expect = torch.matmul((2.0 * qdd.detach()).unsqueeze(-2), Minv).squeeze(-2)
    assert torch.allclose(tau.grad, expect, rtol=1e-5, atol=1e-6 * float(expect.abs().max()))

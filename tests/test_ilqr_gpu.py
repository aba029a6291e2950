"""env.sim.rollout_joint_feedback (dg_world_rollout_feedback / rollout_feedback_kernel) and env.sim.lq_backward_pass
(dg_world_lq_backward / lq_backward_kernel) on the GPU against the fp64 reference of tests/ilqr_ref.py (itself pinned by
tests/test_ilqr_ref.py), and one iLQR iteration through the three calls.

FEEDBACK ROLLOUT.  Scenes of tests/test_fd_gpu.py: the pendulum (n = 1), the branching cart bolted down (n = 3), a UR5 (n = 6) and the
twelve-joint UR5 + gripper tree; (B, K, T) of (1, 1, 1), (3, 4, 8) and (70, 3, 4), the last also with DG_MAX_LANES 4 (the
global-workspace mode: two workgroups for 210 items, every lane strides).  Start states and feed-forward torques as that file draws
them (the torques of accelerations in [-3, 3] at the start state); ``dtau`` the torque change of an acceleration change in [-1, 1] at
the start state (a random +-30 % of each joint's feed-forward, tried first, is a torque no controller asks for: it drives the gripper's
fingers, 1e-6 kg m^2, where the fp32 solve of that tree is 2.7e-4 off, and the call WITHOUT gains measured qd 1.5e-5 at 3 envs and
2.8e-5 at 70 against the open-loop ceiling 1.9e-5 -- the reason the open-loop file gives for its own torques); the references q_ref,
qd_ref the fp64 nominal trajectory of the feed-forward itself, as in the line search the kernel exists for: the feedback then acts
on the deviation alpha dtau causes.  (References a fixed +-0.05 rad off the start make the gains command the gripper's fingers --
1e-6 kg m^2 -- to 3000 rad/s^2, where the fp32 solve of that tree, cond M 1.45e6, is 2.7e-4 off (tests/test_ddq_gpu.py): measured so,
ur5_gripper x3 qd 5.52e-5 against the open-loop ceiling 1.9e-5; the open-loop file keeps its accelerations in [-3, 3] for that reason.)
The gains are random, of the size lq_backward produces for the scene: the fp64
reference's own K_t of ilqr_controller's defaults (its cost, its horizon of 32, its dt of one env step) about one start state, rows
t = 0 .. T-1 -- the rows a receding-horizon controller applies -- each entry times U(0.5, 1) per env and step: random in size, with the
sign of a control law (a random SIGN makes stiff gains double the state error every step: a trajectory that no two precisions share,
as test_fd_gpu says of uniform torques).  The start velocities are redrawn into 1 <= |qd0| <= 2 per joint (the sign kept): the measure below is relative to the item's own
largest entry, and among 70 pendulums drawn in [-2, 2] one starts at |qd| < 0.1 rad/s and has no scale to be relative to -- measured
with the plain draws: pendulum x70 qd 1.02e-5 against the ceiling 2.8e-6 at an absolute error of 1e-6 rad/s, the fp32 error of the
forward-dynamics solve itself, which the open-loop file never meets because its short chains run in batches of 1 and 3.
alphas = [1, 0.5, 0.25, 0.125][:K].  Every case runs
without and with tau_limit: 0.999 x the 99th percentile of the case's unclamped |torque| on the even joints among the first six, 0 (no
limit) on the others: a clamp that shaves the peaks, as an effort limit does.  (A clamp at the MEDIAN takes tens of N m off the
gripper tree's arm joints in half of the rows; the fingers' feed-forward no longer balances the wrist's acceleration, they spin, and
the fp32 solve of that tree then measures qd 7.8e-5 at 70 envs against the open-loop ceiling 1.9e-5 -- its own error, as above; every
other case passed with the median too.)  The
reference is asserted to clamp in at least one row and not in all.
Error measure, as test_fd_gpu: per item (env, sample), max |gpu - reference| over the trajectory / the largest |reference| entry of that
trajectory, for q, qd, pos and tau.  Bounds: 8 x the largest figure measured on an MI355X over all cases of this file (MEASURED_FB),
never above a ceiling fixed beforehand: for q, qd, pos the bound test_fd_gpu asserts for the open-loop rollout of the group; for tau
(no open-loop counterpart) what those state ceilings allow through the gain row plus the rounding of the 2 n + 2 fp32 terms:
    max_ti [ sum_j |g_ij| c_j + (2 n + 3) 2^-24 (|tau_ff| + |alpha dtau| + sum_j |g_ij dx_j|) ] / max |tau|,  c_j = ceiling x max |q| or |qd|.

BACKWARD PASS.  n in {1, 3, 6, 12}; T = 1, T = 8 (P = T) and the stationary P = 1 with T = 100; substeps 1 and 2; B 1 and 70.  The inputs
are the GPU's own forward_dynamics_derivatives at random points, the weights random SPD matrices per env (S S^T / m + I scaled 10 /
1e-3 / 1000 for lxx / luu / lxx_T), once with random lx, lu, lx_T and once without.  Reference: ilqr_ref.lq_backward on the SAME fp32
inputs in fp64; status == 0 on the reference first.  Per env max |K - ref| / max |ref|, likewise k and dV; bound 8 x MEASURED_LQ, never
above 1e-5 (what tests/test_lqr_controller_host.py grants fp32-in / fp64-compute gains).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import ddq_ref as DD
import dynamics_ref as D
import ilqr_ref as IL
import test_fd_gpu as TF
from diy_gym_amd.backend import FeedbackRollout, LqBackward
from test_fd_gpu import DEV, G, GROUP, LOCAL, SCENES, dev, frame_of, make, per_row

pytestmark = pytest.mark.gpu
FB_SCENES = ('pendulum', 'cart_tree', 'ur_admittance', 'ur5_gripper')
ALPHAS = [1.0, 0.5, 0.25, 0.125]
BKT = ((1, 1, 1), (3, 4, 8), (70, 3, 4))
FB_CASES = [(s, B, K, T, None) for s in FB_SCENES for B, K, T in BKT] + [('ur_admittance', 70, 3, 4, '4')]
# measured maxima (MI355X, all cases of this file) and the bounds 8 x them, never above the ceilings
MEASURED_FB = {
    # q: ur_admittance x3 K=4 T=8 with the limit; qd: ur5_gripper x70 K=3 T=4 with the limit; pos: ur_admittance x70 K=3 T=4 (both lane modes the same figures);
    # tau: ur5_gripper x70 K=3 T=4
    'arms': {'q': 2.45e-7, 'qd': 6.78e-6, 'pos': 1.64e-6, 'tau': 4.61e-6},
    # q: cart_tree x3 K=4 T=8; qd: pendulum x3 K=4 T=8 with the limit; pos: cart_tree x70 K=3 T=4; tau: pendulum x70 K=3 T=4 (an item whose torque nearly cancels: a
    # small largest entry)
    'short': {'q': 2.21e-7, 'qd': 9.99e-7, 'pos': 2.70e-7, 'tau': 3.23e-5},
}
# K: cart_tree x70 T=8 substeps 1; k: ur5_gripper x70 T=8 substeps 1; dV: cart_tree x70 T=8 substeps 2 -- the rounding of the fp32 outputs (2^-24 = 5.96e-8)
MEASURED_LQ = {'K': 5.32e-8, 'k': 5.81e-8, 'dV': 5.84e-8}
LQ_CEILING = 1e-5
BOUND_LQ = {k: min(8 * v, LQ_CEILING) for k, v in MEASURED_LQ.items()}
_FB, _GAIN = {}, {}


def fb_bound(group, field, tau_ceiling=None):
    ceiling = tau_ceiling if field == 'tau' else TF.BOUND[group][field]
    return min(8 * MEASURED_FB[group][field], ceiling)


HORIZON = 32   # ilqr_controller's default


def gain_size(scene, T, env, model, q0):
    """K_t [T, n, 2 n], t = 0 .. T-1, of the fp64 backward pass about q0 at rest under gravity compensation: ilqr_controller's default
    cost, horizon and dt."""
    key = (scene, T)
    if key not in _GAIN:
        robot, uid = model.robot, model.uid
        Tb = D.base_transforms(env, uid)[0]
        n = robot.num_dofs
        tau_g = D.inverse_dynamics(robot, q0, np.zeros(n), np.zeros(n), G, Tb)
        d = DD.derivatives(robot, q0, np.zeros(n), tau_g, True, G, Tb)
        lxx, luu, _, _, lxx_T, _ = IL.cost_terms(q0, np.zeros(n), np.tile(q0, (1, 1)), np.zeros((1, n)), np.zeros((1, n)), q0, tau_g)
        b = IL.lq_backward(d.dqdd_dq, d.dqdd_dqd, d.dqdd_dtau, env.layout.dt * env.layout.substeps, lxx, luu, lxx_T, T=HORIZON)
        assert b.status == 0
        _GAIN[key] = b.K[:T]
    return _GAIN[key]


def fb_case(scene, B, K, T, env, model):
    """The inputs of a case (fp32 numpy) and its fp64 reference without a limit: computed once."""
    key = (scene, B, K, T)
    if key not in _FB:
        robot, uid = model.robot, model.uid
        n = robot.num_dofs
        Tb, scales = D.base_transforms(env, uid), D.mass_scales(env, uid)
        q0, qd0, acc = TF.draws(robot, B, 5000 * B + 10 * K + T, (T, ))
        qd0 = (np.where(qd0 < 0, -1.0, 1.0) * (1.0 + 0.5 * np.abs(qd0))).astype(np.float32)   # 1 <= |qd0| <= 2 (module docstring)
        rng = np.random.default_rng(77 * B + 5 * K + T)
        tau_ff = np.stack([[D.inverse_dynamics(robot, q0[e].astype(np.float64), qd0[e], acc[e, t], G, Tb[e], scales[e]) for t in range(T)] for e in range(B)]).astype(np.float32)
        dacc = rng.uniform(-1.0, 1.0, acc.shape)
        dtau = np.stack([[D.inverse_dynamics(robot, q0[e].astype(np.float64), qd0[e], acc[e, t] + dacc[e, t], G, Tb[e], scales[e])
                          - D.inverse_dynamics(robot, q0[e].astype(np.float64), qd0[e], acc[e, t], G, Tb[e], scales[e]) for t in range(T)] for e in range(B)]).astype(np.float32)
        gain = (gain_size(scene, T, env, model, q0[0].astype(np.float64))[None] * rng.uniform(0.5, 1.0, (B, T, n, 2 * n))).astype(np.float32)
        nominal = [IL.feedback_rollout(robot, q0[e], qd0[e], tau_ff[e], env.layout.dt, damping=True, g=G, T_base=Tb[e], scale=scales[e]) for e in range(B)]
        q_ref = np.stack([np.vstack([q0[e][None], nominal[e][0][:-1]]) for e in range(B)]).astype(np.float32)   # the states BEFORE each step
        qd_ref = np.stack([np.vstack([qd0[e][None], nominal[e][1][:-1]]) for e in range(B)]).astype(np.float32)
        ins = dict(q0=q0, qd0=qd0, tau=tau_ff, dtau=dtau, gain=gain, q_ref=q_ref, qd_ref=qd_ref, alphas=np.array(ALPHAS[:K], dtype=np.float32))
        _FB[key] = (ins, fb_reference(scene, ins, None, env, model))
    return _FB[key]


def fb_reference(scene, ins, limit, env, model):
    robot, uid = model.robot, model.uid
    Tb, scales = D.base_transforms(env, uid), D.mass_scales(env, uid)
    B, T, n = ins['tau'].shape
    K = len(ins['alphas'])
    frame = frame_of(robot, SCENES[scene][2])
    out = dict(q=np.zeros((B, K, T, n)), qd=np.zeros((B, K, T, n)), tau=np.zeros((B, K, T, n)), pos=np.zeros((B, K, T, 3)))
    for e in range(B):
        for k in range(K):
            out['q'][e, k], out['qd'][e, k], out['tau'][e, k], out['pos'][e, k] = IL.feedback_rollout(
                robot, ins['q0'][e], ins['qd0'][e], ins['tau'][e], env.layout.dt, ins['gain'][e], ins['q_ref'][e], ins['qd_ref'][e], ins['dtau'][e], ins['alphas'][k], limit,
                True, frame, LOCAL, G, Tb[e], scales[e])
    return out


def fb_call(sim, uid, ins, frame=None, limit=None, want=('q', 'qd', 'tau'), **over):
    a = dict(ins, **over)
    t = lambda v: None if v is None else dev(v)
    return sim.rollout_joint_feedback(uid, t(a['tau']), t(a['gain']), t(a['q_ref']), t(a['qd_ref']), t(a['dtau']), t(a['alphas']), t(a['q0']), t(a['qd0']), frame=frame,
                                      local_pos=LOCAL, joint_damping=True, tau_limit=t(limit), want=want)


def tau_ceiling(group, ins, ref):
    """Per item [B, K]: what the state ceilings allow through the gain rows, plus the rounding of the fp32 sum (module docstring)."""
    B, T, n = ins['tau'].shape
    g = np.abs(ins['gain'].astype(np.float64))
    out = np.zeros(ref['tau'].shape[:2])
    for k, alpha in enumerate(ins['alphas']):
        qs = np.concatenate([ins['q0'][:, None, :], ref['q'][:, k, :-1]], axis=1); qds = np.concatenate([ins['qd0'][:, None, :], ref['qd'][:, k, :-1]], axis=1)
        cq = TF.BOUND[group]['q'] * np.abs(ref['q'][:, k]).max(axis=(1, 2)); cv = TF.BOUND[group]['qd'] * np.abs(ref['qd'][:, k]).max(axis=(1, 2))
        through = g[..., :n].sum(axis=3) * cq[:, None, None] + g[..., n:].sum(axis=3) * cv[:, None, None]
        terms = (np.abs(ins['tau']) + np.abs(alpha * ins['dtau']) + (g[..., :n] * np.abs(qs - ins['q_ref'])[:, :, None, :]).sum(axis=3)
                 + (g[..., n:] * np.abs(qds - ins['qd_ref'])[:, :, None, :]).sum(axis=3))
        out[:, k] = (through + (2 * n + 3) * 2.0 ** -24 * terms).max(axis=(1, 2)) / np.abs(ref['tau'][:, k]).max(axis=(1, 2))
    return out


@pytest.mark.parametrize('limited', [False, True])
@pytest.mark.parametrize('scene,B,K,T,lanes', FB_CASES)
def test_feedback_rollout_matches_the_reference(scene, B, K, T, lanes, limited, monkeypatch):
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n, frame, group = robot.num_dofs, frame_of(robot, SCENES[scene][2]), GROUP[scene]
    ins, ref = fb_case(scene, B, K, T, env, model)
    limit = None
    if limited:
        limit = np.where((np.arange(n) % 2 == 0) & (np.arange(n) < 6), 0.999 * np.quantile(np.abs(ref['tau']).reshape(-1, n), 0.99, axis=0), 0.0).astype(np.float32)
        ref = fb_reference(scene, ins, limit, env, model)
        rows = (np.abs(ref['tau'][..., limit > 0]) == limit[limit > 0]).any(axis=-1)
        assert rows.sum() >= 1 and (~rows).sum() >= (0 if rows.size == 1 else 1), (rows.sum(), rows.size)   # it binds in a row, and not in all
        assert np.abs(ref['tau'][..., limit == 0]).max(initial=0.0) > 0 or n == 1
    before = sim.get_state()
    r = fb_call(sim, uid, ins, frame, limit, want=('q', 'qd', 'tau', 'pos', 'singular'))
    assert isinstance(r, FeedbackRollout) and r.q.shape == r.qd.shape == r.tau.shape == (B, K, T, n) and r.pos.shape == (B, K, T, 3) and r.singular.shape == (B, K)
    assert r.singular.dtype == torch.int32 and bool((r.singular == 0).all()) and all(bool(torch.isfinite(t).all()) for t in (r.q, r.qd, r.tau, r.pos))
    assert np.array_equal(sim.get_state(), before)   # the state is never written
    figs = {f: per_row(getattr(r, f).cpu().numpy().reshape(B * K, -1), ref[f].reshape(B * K, -1)) for f in ('q', 'qd', 'tau', 'pos')}
    ceil = tau_ceiling(group, ins, ref).reshape(-1)
    print('FB %s x%d K=%d T=%d lanes=%s limited=%s grid=%d: %s (tau ceiling %.3g .. %.3g)' % (scene, B, K, T, sim.lanes, limited, sim.rollout_grid(K),
          ' '.join('%s %.4g' % (f, v.max()) for f, v in figs.items()), ceil.min(), ceil.max()))
    for f in ('q', 'qd', 'pos'):
        assert figs[f].max() < fb_bound(group, f), (scene, f, figs[f].max(), fb_bound(group, f))
    assert (figs['tau'] < np.minimum(8 * MEASURED_FB[group]['tau'], ceil)).all(), (scene, figs['tau'].max(), ceil.min())
    if limited:
        lim = dev(limit)
        assert bool((r.tau.abs()[..., lim > 0] <= lim[lim > 0]).all()) and bool((r.tau.abs()[..., lim > 0] == lim[lim > 0]).any())
    if lanes:   # the capped grid strides: the last stride's items were computed too
        assert sim.rollout_grid(K) == (B + 63) // 64 < (B * K + 63) // 64 and figs['q'][-10:].max() > 0


@pytest.mark.parametrize('scene,B,K,T,lanes', [('pendulum', 3, 4, 8, None), ('cart_tree', 3, 4, 8, None), ('ur_admittance', 3, 4, 8, None), ('ur5_gripper', 3, 4, 8, None),
                                               ('ur_admittance', 70, 3, 4, '4')])
def test_feedback_rollout_identities_in_bits(scene, B, K, T, lanes, monkeypatch):
    env, model = make(scene, B, lanes, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    n, frame = robot.num_dofs, frame_of(robot, SCENES[scene][2])
    ins, _ = fb_case(scene, B, K, T, env, model)
    every = ('q', 'qd', 'tau', 'pos', 'singular')
    keep = lambda r: FeedbackRollout(*[None if t is None else t.clone() for t in r])
    # (i) tau alone is the open-loop rollout of tau repeated over K; (ii) all-zero gain and dtau the same
    tau4 = np.ascontiguousarray(np.broadcast_to(ins['tau'][:, None], (B, K, T, n)))
    open_loop = [t.clone() for t in sim.rollout_joint_dynamics(uid, dev(tau4), dev(ins['q0']), dev(ins['qd0']), frame=frame, local_pos=LOCAL, joint_damping=True,
                                                               want=('q', 'qd', 'pos', 'singular'))]
    bare = keep(fb_call(sim, uid, ins, frame, want=every, gain=None, q_ref=None, qd_ref=None, dtau=None))
    zeros = keep(fb_call(sim, uid, ins, frame, want=every, gain=np.zeros_like(ins['gain']), dtau=np.zeros_like(ins['dtau'])))
    for r in (bare, zeros):
        assert all(torch.equal(a, b) for a, b in zip(open_loop, (r.q, r.qd, r.pos, r.singular)))
        assert torch.equal(r.tau, dev(tau4))
    assert float(bare.q.abs().max()) > 0
    # (iii) sample k of a K-sample call is the one-sample call given alphas[k]
    full = keep(fb_call(sim, uid, ins, frame, want=every))
    assert not torch.equal(full.q, bare.q)
    for k in range(K):
        one = fb_call(sim, uid, ins, frame, want=every, alphas=ins['alphas'][k:k + 1])
        assert all(torch.equal(a[:, k:k + 1], b) for a, b in zip(full, one)), k
    # (iv) q0 = None is the env's own state
    sim.reset_joint_state(uid, dev(ins['q0']), dev(ins['qd0']))
    q, qd = (t.clone() for t in sim.joint_states(uid))
    assert torch.equal(q, dev(ins['q0']))
    own = fb_call(sim, uid, ins, frame, want=every, q0=None, qd0=None)
    assert all(torch.equal(a, b) for a, b in zip(full, own))
    # (v) tau_out without a limit and with zero gains is tau_ff + alpha dtau as torch computes it
    r = fb_call(sim, uid, ins, frame, want=('tau', ), gain=np.zeros_like(ins['gain']))
    expect = dev(ins['tau'])[:, None] + dev(ins['alphas'])[None, :, None, None] * dev(ins['dtau'])[:, None]
    assert torch.equal(r.tau, expect)
    # (vi) every subset of want gives the bits of the full call
    for mask in range(1, 32):
        want = tuple(f for i, f in enumerate(every) if mask >> i & 1)
        sub = fb_call(sim, uid, ins, frame if 'pos' in want else None, want=want)
        for f in every:
            assert (getattr(sub, f) is None) == (f not in want)
            assert getattr(sub, f) is None or torch.equal(getattr(sub, f), getattr(full, f)), (want, f)
    a, b = fb_call(sim, uid, ins), fb_call(sim, uid, ins, dtau=0.5 * ins['dtau'])
    assert a.q.data_ptr() == b.q.data_ptr() and a.pos is None and a.singular is None   # buffers kept per (want, K, T) and reused


def test_feedback_refusals_raise_value_error_with_the_entrys_text_and_launch_nothing(monkeypatch):
    env, model = make('cart_tree', 3, None, monkeypatch)
    sim, robot, uid = env.sim, model.robot, model.uid
    ins, _ = fb_case('cart_tree', 3, 4, 8, env, model)
    tip = frame_of(robot, 'tip_joint')
    kept = [t for t in fb_call(sim, uid, ins, tip, want=('q', 'qd', 'tau', 'pos', 'singular'))]
    before = [t.clone() for t in kept]
    R = 'dg_world_rollout_feedback: '
    tau, gain, ref, dtau = dev(ins['tau']), dev(ins['gain']), dev(ins['q_ref']), dev(ins['dtau'])
    call = sim.rollout_joint_feedback
    bad = [(lambda: call(99, tau), 'out of range'),
           (lambda: call(uid, None), R + 'tau_ff is NULL'),
           (lambda: call(uid, tau[:, :0].contiguous()), R + 'T must be >= 1, got 0'),
           (lambda: call(uid, tau, dtau=dtau, alphas=[]), R + 'K must be >= 1, got 0'),
           (lambda: call(uid, tau, dt=0.0), R + 'dt must be finite and > 0, got 0'),
           (lambda: call(uid, tau, dt=float('nan')), R + 'dt must be finite and > 0, got nan'),
           (lambda: call(uid, tau, dt=float('inf')), R + 'dt must be finite and > 0, got inf'),
           (lambda: call(uid, tau, dtau=dtau), R + 'dtau needs alpha'),
           (lambda: call(uid, tau, gain=gain), R + 'gain needs q_ref and qd_ref'),
           (lambda: call(uid, tau, gain=gain, q_ref=ref), R + 'gain needs q_ref and qd_ref'),
           (lambda: call(uid, tau, gain=gain, qd_ref=ref), R + 'gain needs q_ref and qd_ref'),
           (lambda: call(uid, tau, want=()), R + 'every output is NULL'),
           (lambda: call(uid, tau, want=('pos', )), "'pos' in want needs frame"),
           (lambda: call(uid, tau, frame=len(robot.joints), want=('pos', )), R + 'body %d has no frame %d' % (uid, len(robot.joints))),
           (lambda: call(uid, tau, frame=tip, local_pos=(0.0, 0.0), want=('pos', )), 'local_pos'),
           (lambda: call(uid, tau, want=('torque', )), 'want'),
           (lambda: call(uid, tau[:, :, :2].contiguous()), 'shape'),
           (lambda: call(uid, tau[:2].contiguous()), 'shape'),
           (lambda: call(uid, tau, gain=gain[..., :3].contiguous(), q_ref=ref, qd_ref=ref), 'shape'),
           (lambda: call(uid, tau, gain=gain, q_ref=ref[:, :2].contiguous(), qd_ref=ref), 'shape'),
           (lambda: call(uid, tau, tau_limit=[1.0, 2.0]), 'shape'),
           (lambda: call(uid, tau.double()), 'float32'),
           (lambda: call(uid, tau.cpu()), 'cpu')]
    for fn, text in bad:
        with pytest.raises(ValueError) as info:
            fn()
        assert text in str(info.value), (text, str(info.value))
    lib, st = sim.lib, ctypes.c_void_p(sim.state.data_ptr())
    out = torch.full((3, 256), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    o, lp, t, g, r, d, al = p(out), (ctypes.c_float * 3)(*LOCAL), p(tau), p(gain), p(ref), p(dtau), p(dev(ins['alphas']))
    big = 2 ** 31 - 1
    N = None
    for args, text in (((None, st, uid, tip, lp, 2, 4, 0.01, 0, N, N, t, N, N, N, N, N, N, o, o, o, o, o), 'null argument'),
                       ((sim.handle, N, uid, tip, lp, 2, 4, 0.01, 0, N, N, t, N, N, N, N, N, N, o, o, o, o, o), 'null argument'),
                       ((sim.handle, st, uid, tip, lp, 0, 4, 0.01, 0, N, N, t, N, N, N, N, N, N, o, o, o, o, o), 'K must be >= 1, got 0'),
                       ((sim.handle, st, uid, tip, lp, 2, -1, 0.01, 0, N, N, t, N, N, N, N, N, N, o, o, o, o, o), 'T must be >= 1, got -1'),
                       ((sim.handle, st, uid, tip, lp, 2, 4, 0.0, 0, N, N, t, N, N, N, N, N, N, o, o, o, o, o), 'dt must be finite and > 0, got 0'),
                       ((sim.handle, st, uid, tip, lp, 2, 4, 0.01, 0, N, N, N, N, N, N, N, N, N, o, o, o, o, o), 'tau_ff is NULL'),
                       ((sim.handle, st, uid, tip, lp, 2, 4, 0.01, 0, N, N, t, d, N, N, N, N, N, o, o, o, o, o), 'dtau needs alpha'),
                       ((sim.handle, st, uid, tip, lp, 2, 4, 0.01, 0, N, N, t, d, al, g, r, N, N, o, o, o, o, o), 'gain needs q_ref and qd_ref'),
                       ((sim.handle, st, uid, tip, lp, 2, 4, 0.01, 0, N, N, t, N, N, N, N, N, N, N, N, N, N, N), 'every output is NULL'),
                       ((sim.handle, st, uid, tip, lp, big, big, 0.01, 0, N, N, t, N, N, N, N, N, N, o, o, o, o, o), '3 envs x K %d x T %d x 3 joints is beyond INT64_MAX / 4 values' % (big, big)),
                       ((sim.handle, st, uid, tip, N, 2, 4, 0.01, 0, N, N, t, N, N, N, N, N, N, o, o, o, o, o), 'local_pos is NULL'),
                       ((sim.handle, st, uid, -1, lp, 2, 4, 0.01, 0, N, N, t, N, N, N, N, N, N, o, o, o, o, o), 'frame -1 out of range')):
        assert lib.dg_world_rollout_feedback(*args, None) == -4
        assert lib.dg_last_error().decode().startswith('dg_world_rollout_feedback: ' + text), (text, lib.dg_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and all(torch.equal(a, b) for a, b in zip(kept, before))   # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- backward pass
LQ_SCENES = {'pendulum': 1, 'cart_tree': 3, 'ur_admittance': 6, 'ur5_gripper': 12}
LQ_CASES = [(s, B, T, P, sub) for s in LQ_SCENES for B, T, P, sub in ((1, 1, 1, 1), (70, 1, 1, 2), (1, 8, 8, 1), (70, 8, 8, 2), (1, 8, 8, 2), (70, 8, 8, 1), (1, 100, 1, 1),
                                                                     (70, 100, 1, 2))]
_LQ_POOL = {}


def spd(rng, B, m, scale):
    S = rng.uniform(-1.0, 1.0, (B, m, m))
    return (scale * (S @ S.transpose(0, 2, 1) / m + np.eye(m))).astype(np.float32)


def lq_inputs(scene, B, P, sim, model):
    """The GPU's own derivatives at B x P random points (fp32 numpy) and random SPD weights per env."""
    key = (scene, B, P)
    if key not in _LQ_POOL:
        robot, uid = model.robot, model.uid
        n = robot.num_dofs
        q, qd, tau = TF.draws(robot, B * P, 900 + 7 * B + P)
        shape = (B, P, n)
        d = sim.forward_dynamics_derivatives(uid, dev(q.reshape(shape)), dev(qd.reshape(shape)), dev(tau.reshape(shape)), joint_damping=True,
                                             want=('dqdd_dq', 'dqdd_dqd', 'dqdd_dtau', 'singular'))
        assert bool((d.singular == 0).all())
        rng = np.random.default_rng(31 * B + P)
        _LQ_POOL[key] = dict(A_q=d.dqdd_dq.cpu().numpy().copy(), A_v=d.dqdd_dqd.cpu().numpy().copy(), Minv=d.dqdd_dtau.cpu().numpy().copy(),
                             lxx=spd(rng, B, 2 * n, 10.0), luu=spd(rng, B, n, 1e-3), lxx_T=spd(rng, B, 2 * n, 1000.0))
    return _LQ_POOL[key]


def lq_figures(got, ref):
    """Per env max |got - ref| / max |ref| of K, k, dV against a list of reference LqBackward."""
    out = {}
    for f in ('K', 'k', 'dV'):
        g = getattr(got, f).cpu().numpy().astype(np.float64)
        r = np.stack([getattr(b, f) for b in ref])
        scale = np.abs(r.reshape(len(ref), -1)).max(axis=1)
        err = np.abs((g - r).reshape(len(ref), -1)).max(axis=1)
        assert (err[scale == 0] == 0).all()
        out[f] = float(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0).max())
    return out


@pytest.mark.parametrize('scene,B,T,P,substeps', LQ_CASES)
def test_backward_pass_matches_the_reference(scene, B, T, P, substeps, monkeypatch):
    env, model = make(scene, B, None, monkeypatch)
    sim, uid, n = env.sim, model.uid, model.robot.num_dofs
    m, dt = 2 * n, env.layout.dt
    a = lq_inputs(scene, B, P, sim, model)
    rng = np.random.default_rng(5 * T + substeps)
    grads = dict(lx=rng.uniform(-1.0, 1.0, (B, T, m)).astype(np.float32), lu=rng.uniform(-0.01, 0.01, (B, T, n)).astype(np.float32),
                 lx_T=rng.uniform(-10.0, 10.0, (B, m)).astype(np.float32))
    for with_grads in (True, False):
        g = grads if with_grads else dict(lx=None, lu=None, lx_T=None)
        ref = [IL.lq_backward(a['A_q'][e], a['A_v'][e], a['Minv'][e], dt, a['lxx'][e], a['luu'][e], a['lxx_T'][e], None if g['lx'] is None else g['lx'][e],
                              None if g['lu'] is None else g['lu'][e], None if g['lx_T'] is None else g['lx_T'][e], 0.0, T, substeps) for e in range(B)]
        assert all(b.status == 0 for b in ref)   # on the reference first
        t = lambda v: None if v is None else dev(v)
        got = sim.lq_backward_pass(uid, dev(a['A_q']), dev(a['A_v']), dev(a['Minv']), dt, dev(a['lxx']), dev(a['luu']), dev(a['lxx_T']), t(g['lx']), t(g['lu']), t(g['lx_T']),
                                   horizon=T, substeps=substeps)
        assert isinstance(got, LqBackward) and got.K.shape == (B, T, n, m) and got.k.shape == (B, T, n) and got.dV.shape == (B, 2) and got.status.shape == (B, )
        assert got.status.dtype == torch.int32 and bool((got.status == 0).all()) and all(bool(torch.isfinite(x).all()) for x in (got.K, got.k, got.dV))
        figs = lq_figures(got, ref)
        print('LQ %s x%d T=%d P=%d substeps=%d grads=%s: %s' % (scene, B, T, P, substeps, with_grads, ' '.join('%s %.4g' % kv for kv in figs.items())))
        for f, v in figs.items():
            assert v < BOUND_LQ[f], (scene, f, v, BOUND_LQ[f])
        if not with_grads:
            assert float(got.k.abs().max()) == 0 and float(got.dV.abs().max()) == 0
    if P == 1 and T > 1:   # P = 1 equals P = T given T copies, in bits
        keep = [x.clone() for x in got]
        rep = lambda v: dev(np.ascontiguousarray(np.broadcast_to(v, (B, T) + v.shape[2:])))
        copies = sim.lq_backward_pass(uid, rep(a['A_q']), rep(a['A_v']), rep(a['Minv']), dt, dev(a['lxx']), dev(a['luu']), dev(a['lxx_T']), substeps=substeps)
        assert all(torch.equal(x, y) for x, y in zip(keep, copies))
        per_step = sim.lq_backward_pass(uid, dev(a['A_q']), dev(a['A_v']), dev(a['Minv']), dt, rep(a['lxx'][:, None]), rep(a['luu'][:, None]), dev(a['lxx_T']), horizon=T,
                                        substeps=substeps)
        assert all(torch.equal(x, y) for x, y in zip(keep, per_step))


def test_an_indefinite_quu_is_reported_with_zeros_and_mu_clears_it(monkeypatch):
    B, T = 3, 5
    env, model = make('ur_admittance', B, None, monkeypatch)
    sim, uid, n = env.sim, model.uid, 6
    a = lq_inputs('ur_admittance', B, 1, sim, model)
    dt = env.layout.dt
    zero_R, zero_T = torch.zeros((n, n), device=DEV), torch.zeros((2 * n, 2 * n), device=DEV)
    dyn = [dev(a[k]) for k in ('A_q', 'A_v', 'Minv')]
    lx = dev(np.ones((B, 2 * n), dtype=np.float32))
    # luu = 0 and lxx_T = 0: Quu of step T - 1 is the zero matrix
    sim.lq_backward_pass(uid, *dyn, dt, dev(a['lxx']), dev(a['luu']), dev(a['lxx_T']), lx, horizon=T)   # (fills the buffers with something else first)
    bad = sim.lq_backward_pass(uid, *dyn, dt, dev(a['lxx']), zero_R, zero_T, lx, horizon=T)
    assert bad.status.tolist() == [T] * B and all(float(x.abs().max()) == 0 for x in (bad.K, bad.k, bad.dV))
    ok = sim.lq_backward_pass(uid, *dyn, dt, dev(a['lxx']), zero_R, zero_T, lx, mu=1e-3, horizon=T)
    ref = [IL.lq_backward(a['A_q'][e], a['A_v'][e], a['Minv'][e], dt, a['lxx'][e], np.zeros((n, n)), np.zeros((2 * n, 2 * n)), np.ones(2 * n), mu=float(np.float32(1e-3)), T=T)
           for e in range(B)]
    assert all(b.status == 0 for b in ref) and ok.status.tolist() == [0] * B and all(bool(torch.isfinite(x).all()) for x in (ok.K, ok.k, ok.dV))
    figs = lq_figures(ok, ref)
    print('LQ mu: %s' % figs)
    assert all(v < BOUND_LQ[f] for f, v in figs.items()), figs
    # only env 1 of 3 indefinite: envs 0 and 2 are their one-env calls in bits
    luu = np.stack([a['luu'][0], np.zeros((n, n), dtype=np.float32), a['luu'][2]]); lxx_T = np.stack([a['lxx_T'][0], np.zeros((2 * n, 2 * n), dtype=np.float32), a['lxx_T'][2]])
    mixed = [x.clone() for x in sim.lq_backward_pass(uid, *dyn, dt, dev(a['lxx']), dev(luu), dev(lxx_T), lx, horizon=T)]
    assert mixed[3].tolist() == [0, T, 0] and all(float(x[1].abs().max()) == 0 for x in mixed[:3]) and all(bool(torch.isfinite(x).all()) for x in mixed[:3])
    one_env, one_model = make('ur_admittance', 1, None, monkeypatch)
    for e in (0, 2):
        row = lambda v: dev(v[e:e + 1])
        one = one_env.sim.lq_backward_pass(one_model.uid, row(a['A_q']), row(a['A_v']), row(a['Minv']), dt, row(a['lxx']), row(luu), row(lxx_T), lx[e:e + 1].contiguous(), horizon=T)
        assert all(torch.equal(x[e:e + 1], y) for x, y in zip(mixed, one)), e
    # a NaN in the inputs is a failure, not a NaN in the outputs
    poisoned = a['Minv'].copy(); poisoned[1, 0, 2, 3] = np.nan
    r = sim.lq_backward_pass(uid, dyn[0], dyn[1], dev(poisoned), dt, dev(a['lxx']), dev(a['luu']), dev(a['lxx_T']), lx, horizon=T)
    assert r.status.tolist() == [0, T, 0] and all(bool(torch.isfinite(x).all()) for x in (r.K, r.k, r.dV)) and float(r.K[1].abs().max()) == 0
    # ... also one that never meets a pivot: Quu is made of B and Vxx alone, so a NaN in A_q or an Inf in lx leaves it finite
    # (a gradient of step t enters Vx there and Qu, hence k, one step later: lx fails at step T - 2, and with T = 1 it reaches no output)
    for key, where, value, horizon, status in (('A_q', (1, 0, 0, 0), np.nan, T, T), ('A_q', (1, 0, 0, 0), np.inf, 1, 1), ('A_v', (1, 0, 3, 2), np.nan, T, T),
                                               ('lx', (1, 4), np.inf, T, T - 1), ('lx', (1, 4), np.nan, 1, 0)):
        args = dict(A_q=a['A_q'].copy(), A_v=a['A_v'].copy(), lx=np.ones((B, 2 * n), dtype=np.float32))
        args[key][where] = value
        r = sim.lq_backward_pass(uid, dev(args['A_q']), dev(args['A_v']), dyn[2], dt, dev(a['lxx']), dev(a['luu']), dev(a['lxx_T']), dev(args['lx']), horizon=horizon)
        assert r.status.tolist() == [0, status, 0], (key, value, r.status.tolist())
        assert all(bool(torch.isfinite(x).all()) for x in (r.K, r.k, r.dV)) and float(r.K[0].abs().max()) > 0
        assert (float(r.K[1].abs().max()) == 0) == (status != 0) and (status == 0 or float(r.dV[1].abs().max()) == float(r.k[1].abs().max()) == 0)


def test_backward_refusals_raise_value_error_with_the_entrys_text_and_launch_nothing(monkeypatch):
    B, T = 3, 4
    env, model = make('cart_tree', B, None, monkeypatch)
    sim, uid, n = env.sim, model.uid, 3
    a = {k: dev(v) for k, v in lq_inputs('cart_tree', B, T, sim, model).items()}
    dt = env.layout.dt
    kept = [x for x in sim.lq_backward_pass(uid, a['A_q'], a['A_v'], a['Minv'], dt, a['lxx'], a['luu'], a['lxx_T'])]
    before = [x.clone() for x in kept]
    R = 'dg_world_lq_backward: '
    call = lambda **kw: sim.lq_backward_pass(uid, **dict(dict(a, dt=dt), **kw))
    bad = [(lambda: sim.lq_backward_pass(99, a['A_q'], a['A_v'], a['Minv'], dt, a['lxx'], a['luu'], a['lxx_T']), 'out of range'),
           (lambda: call(horizon=5), R + 'P must be 1 or T = 5, got 4'),
           (lambda: call(substeps=0), R + 'substeps must be >= 1, got 0'),
           (lambda: call(dt=0.0), R + 'dt must be finite and > 0, got 0'),
           (lambda: call(dt=float('nan')), R + 'dt must be finite and > 0, got nan'),
           (lambda: call(dt=float('inf')), R + 'dt must be finite and > 0, got inf'),
           (lambda: call(lxx=None), R + 'lxx, luu and lxx_T are required'),
           (lambda: call(lxx_T=None), R + 'lxx, luu and lxx_T are required'),
           (lambda: call(lxx=a['lxx'][:, None].expand(B, 3, 6, 6).contiguous()), "the cost's P must be 1 or T = 4, got 3"),
           (lambda: call(A_q=a['A_q'][:, :2].contiguous()), 'A_q, A_v and Minv must all be'),
           (lambda: call(A_q=a['A_q'][:, :, :2].contiguous()), 'shape'),
           (lambda: call(luu=a['luu'][:2].contiguous()), 'shape'),
           (lambda: call(lx=torch.zeros((B, T, 5), device=DEV)), 'shape'),
           (lambda: call(mu=torch.zeros((B + 1, ), device=DEV)), 'shape'),
           (lambda: call(want=('P', )), 'want'),
           (lambda: call(A_q=a['A_q'].double()), 'float32'),
           (lambda: call(A_q=a['A_q'].cpu()), 'cpu')]
    for fn, text in bad:
        with pytest.raises(ValueError) as info:
            fn()
        assert text in str(info.value), (text, str(info.value))
    big_env, big_model = make('ur5_gripper', 1, None, monkeypatch)
    lib = sim.lib
    out = torch.full((B, 1024), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    o, x = p(out), p(a['A_q'])
    N = None
    for args, text in (((None, uid, T, T, 1, 1, dt, x, x, x, x, x, N, N, x, N, N, o, o, o, o), 'null argument'),
                       ((sim.handle, 99, T, T, 1, 1, dt, x, x, x, x, x, N, N, x, N, N, o, o, o, o), 'body 99 out of range'),
                       ((sim.handle, uid, 0, 1, 1, 1, dt, x, x, x, x, x, N, N, x, N, N, o, o, o, o), 'T must be >= 1, got 0'),
                       ((sim.handle, uid, T, 2, 1, 1, dt, x, x, x, x, x, N, N, x, N, N, o, o, o, o), 'P must be 1 or T = 4, got 2'),
                       ((sim.handle, uid, T, T, 3, 1, dt, x, x, x, x, x, N, N, x, N, N, o, o, o, o), "the cost's P must be 1 or T = 4, got 3"),
                       ((sim.handle, uid, T, T, 1, 0, dt, x, x, x, x, x, N, N, x, N, N, o, o, o, o), 'substeps must be >= 1, got 0'),
                       ((sim.handle, uid, T, T, 1, 1, -1.0, x, x, x, x, x, N, N, x, N, N, o, o, o, o), 'dt must be finite and > 0, got -1'),
                       ((sim.handle, uid, T, T, 1, 1, dt, N, x, x, x, x, N, N, x, N, N, o, o, o, o), 'A_q, A_v and Minv are required'),
                       ((sim.handle, uid, T, T, 1, 1, dt, x, x, x, x, N, N, N, x, N, N, o, o, o, o), 'lxx, luu and lxx_T are required'),
                       ((sim.handle, uid, T, T, 1, 1, dt, x, x, x, x, x, N, N, x, N, N, o, o, o, N), 'status is NULL'),
                       ((big_env.sim.handle, big_env.models['plane'].uid, T, T, 1, 1, dt, x, x, x, x, x, N, N, x, N, N, o, o, o, o), 'body %d has no joints' % big_env.models['plane'].uid)):
        assert lib.dg_world_lq_backward(*args, None) == -4
        assert lib.dg_last_error().decode().startswith(R + text), (text, lib.dg_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and all(torch.equal(x, y) for x, y in zip(kept, before))   # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- together
def test_two_ilqr_iterations_through_the_three_calls_predict_their_decrease(monkeypatch):
    """(d) of tests/test_ilqr_ref.py on the GPU: nominal rollout, derivatives along it, backward pass, line search over four alphas.
    The fp64 loop goes 210.250000 -> 95.392749 -> 95.238497; the actual / predicted ratio of both iterations must lie in [0.9, 1.1]
    (fp32 trajectories resolve the 0.154 of the second iteration; the 1.3e-4 of a third they do not, so it is not asserted)."""
    env, model = make('ur_admittance', 1, None, monkeypatch)
    sim, uid = env.sim, model.uid
    T, dt, w = 16, 1.0 / 120.0, IL.WEIGHTS
    q_star = np.array([0.3, -1.0, 1.2, -0.5, 0.4, 0.1])
    q0 = (q_star + np.array([0.3, -0.2, 0.25, 0.2, -0.3, 0.2])).astype(np.float32)[None]
    qd0 = np.zeros((1, 6), dtype=np.float32)
    tau_g = sim.calculate_inverse_dynamics(uid, q=dev(q0), qd=dev(qd0)).clone()
    U = tau_g[:, None, :].expand(1, T, 6).contiguous()
    g64 = tau_g.cpu().numpy()[0].astype(np.float64)
    np64 = lambda t: t.cpu().numpy().astype(np.float64)
    costs, ratios = [], []
    for it in range(2):
        nom = sim.rollout_joint_feedback(uid, U, q0=dev(q0), qd0=dev(qd0), dt=dt, joint_damping=True)
        q, qd, u = np64(nom.q[0, 0]), np64(nom.qd[0, 0]), np64(nom.tau[0, 0])
        c0 = IL.cost(q0[0], qd0[0], q, qd, u, q_star, g64, w)
        qs, qds = torch.cat([dev(q0)[:, None], nom.q[:, 0, :-1]], dim=1), torch.cat([dev(qd0)[:, None], nom.qd[:, 0, :-1]], dim=1)
        un = nom.tau[:, 0].clone()
        d = sim.forward_dynamics_derivatives(uid, qs, qds, un, joint_damping=True)
        terms = IL.cost_terms(q0[0], qd0[0], q, qd, u, q_star, g64, w)
        lxx, luu, lx, lu, lxx_T, lx_T = (dev(x.astype(np.float32)) for x in terms)
        back = sim.lq_backward_pass(uid, d.dqdd_dq, d.dqdd_dqd, d.dqdd_dtau, dt, lxx, luu, lxx_T, lx[None], lu[None], lx_T[None])
        assert back.status.tolist() == [0]
        dV = np64(back.dV[0])
        line = sim.rollout_joint_feedback(uid, un, back.K, qs, qds, back.k, ALPHAS, dev(q0), dev(qd0), dt=dt, joint_damping=True)
        c = [IL.cost(q0[0], qd0[0], np64(line.q[0, k]), np64(line.qd[0, k]), np64(line.tau[0, k]), q_star, g64, w) for k in range(4)]
        costs += [c0, c[0]] if it == 0 else [c[0]]
        ratios.append((c0 - c[0]) / -(dV[0] + dV[1]))
        assert c[0] < c0   # alpha = 1 is taken, as in fp64
        U = line.tau[:, 0].clone()
    print('iLQR on the GPU: costs %s, actual / predicted %s' % (['%.6f' % v for v in costs], ['%.4f' % r for r in ratios]))
    assert abs(costs[0] / 210.25 - 1.0) < 1e-5 and abs(costs[1] / 95.392749 - 1.0) < 1e-3 and abs(costs[2] / 95.238497 - 1.0) < 1e-3
    assert all(0.9 <= r <= 1.1 for r in ratios), ratios

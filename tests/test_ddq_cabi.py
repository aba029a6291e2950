"""The C ABI of the forward-dynamics derivatives (include/diygym_hip.h): declared, typed by the binding, exported, refusing a NULL
world without touching a device; and every scene the GPU tests run the kernel on fits the workspace its world has -- the layout
borrows the transient region and the planner is not touched.  Runs without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DG_ERR_ARG = -4
vp, i32 = ctypes.c_void_p, ctypes.c_int32
NAME = 'dg_world_dynamics_derivatives'
PARAMS = ['dg_world* w', 'const float* state', 'int32_t body', 'int32_t P', 'const float* q', 'const float* qd', 'const float* tau', 'int32_t joint_damping',
          'float* qdd', 'float* dqdd_dq', 'float* dqdd_dqd', 'float* dqdd_dtau', 'float* dtau_dq', 'float* dtau_dqd', 'int32_t* singular', 'void* stream']
ARGTYPES = [vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
SCENES = ['pendulum.yaml', 'double_pendulum.yaml', 'cart_tree_fixed.yaml', 'ur_admittance.yaml', 'ur_randomized.yaml', 'ur5_gripper.yaml',
          os.path.join('derivs', 'ur_lqr.yaml'), os.path.join('derivs', 'ur_free.yaml')]
EXAMPLES = [os.path.join('ur_high_5', 'ur_high_5.yaml'), os.path.join('ur_high_5', 'lqr', 'ur_high_5_lqr.yaml')]


def test_header_declares_the_entry_and_the_binding_types_it():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'diygym_hip.h')).read(), flags=re.S)
    decl = re.search(r'\bint32_t\s+%s\s*\(([^)]*)\)\s*;' % NAME, text)
    assert decl, NAME
    assert [' '.join(p.split()) for p in decl.group(1).split(',')] == PARAMS
    from diy_gym_amd import backend
    res, argtypes = backend.SYMBOLS[NAME]
    assert res is i32 and argtypes == ARGTYPES
    # the outputs, in the entry's order
    assert backend.DynamicsDerivatives._fields == ('qdd', 'dqdd_dq', 'dqdd_dqd', 'dqdd_dtau', 'dtau_dq', 'dtau_dqd', 'singular')
    assert callable(backend.HipBackend.forward_dynamics_derivatives) and callable(backend.HipBackend.forward_dynamics_fn)
    assert 'FIRST derivatives only' in backend.HipBackend.forward_dynamics_fn.__doc__
    assert NAME in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


def test_library_exports_it_and_it_refuses_a_null_world():
    lib = ctypes.CDLL(LIB)
    lib.dg_last_error.restype = ctypes.c_char_p
    fn = getattr(lib, NAME)   # AttributeError: not exported
    fn.restype, fn.argtypes = i32, ARGTYPES
    assert fn(None, None, 0, 1, None, None, None, 0, None, None, None, None, None, None, None, None) == DG_ERR_ARG
    assert lib.dg_last_error() == b'dg_world_dynamics_derivatives: null argument'


def ddq_slots():
    """``ddq_slots(n)`` as diy_gym_amd/csrc/dg_ddq.h defines it, evaluated here: the slots kept throughout plus the larger of the
    tangent phase (nominal + tangent Newton-Euler blocks) and the joint-inertia phase of dg_fdq.h with the n residual slots behind it."""
    text = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_ddq.h')).read()
    fdq = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_fdq.h')).read()
    dynq = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_dynq.h')).read()
    consts = {name: int(re.search(r'\b%s = (\d+)\b' % name, dynq).group(1)) for name in ('DQ_ID_STRIDE', 'DQ_CR_STRIDE')}
    parts = {}
    for name, src in (('ddq_keep', text), ('ddq_tangent', text), ('fdq_inertia', fdq)):
        body = re.search(r'constexpr int %s\(int n\) \{ return ([^;?]*); \}' % name, src).group(1)
        assert re.fullmatch(r'[\w\s+*/()]+', body), body
        parts[name] = body.replace('/', '//')
    assert 'constexpr int ddq_refine(int n) { return fdq_inertia(n) + n; }' in text
    assert 'constexpr int ddq_slots(int n) { return ddq_keep(n) + (ddq_tangent(n) > ddq_refine(n) ? ddq_tangent(n) : ddq_refine(n)); }' in text
    part = lambda name, n: eval(parts[name], {'__builtins__': {}}, dict(consts, n=n))
    return lambda n: part('ddq_keep', n) + max(part('ddq_tangent', n), part('fdq_inertia', n) + n)


def test_the_layout_fits_what_the_planner_guarantees():
    """12 + 32 n for every n <= 12 (at 12 exactly); the figures of DESIGN's slot table; never below the forward-dynamics pass the
    kernel starts with."""
    slots = ddq_slots()
    for n in range(1, 13):
        assert slots(n) <= 12 + 32 * n, (n, slots(n))
    assert slots(13) > 12 + 32 * 13
    assert [slots(n) for n in (1, 2, 3, 6, 10, 12)] == [33, 66, 99, 198, 330, 396]
    import test_fd_cabi
    fdq = test_fd_cabi.fdq_slots()
    assert all(slots(n) >= fdq(n) for n in range(1, 65))


@pytest.mark.parametrize('max_lanes', [None, '4', '1'])
def test_every_scene_of_the_gpu_tests_fits_its_worlds_transient_region(max_lanes, monkeypatch):
    """pendulum, double_pendulum, cart_tree_fixed, ur_admittance, ur_randomized, ur5_gripper, the LQR fixtures and ur_high_5 with its
    LQR example, planned at 1, 70 and 16 384 envs in the default workspace mode and in the narrow modes the GPU tests pin (the C
    entry refuses a body that does not fit: none of these may come to that)."""
    from diy_gym_amd import DIYGym
    from diy_gym_amd.backend import debug_plan
    from oracle_backend import OracleBackend
    import diy_gym_amd.examples  # noqa: F401
    slots = ddq_slots()
    if max_lanes:
        monkeypatch.setenv('DG_MAX_LANES', max_lanes)
    seen, joints = 0, set()
    for cfg in [os.path.join(GOLDEN, s) for s in SCENES] + [os.path.join(ROOT, 'examples', s) for s in EXAMPLES]:
        L = DIYGym(cfg, num_envs=2, backend_factory=OracleBackend).layout
        for B in (1, 70, 16384):
            plan = debug_plan(L, B)
            for b in range(L.n_bodies):
                n = L.body_n_links[b]
                if L.body_fixed[b] and n >= 1:
                    seen += 1
                    joints.add(int(n))
                    assert slots(n) <= plan['tr_slots'], (cfg, B, plan['lanes'], b, n, slots(n), plan['tr_slots'])
    assert seen >= 3 * len(SCENES) and {1, 2, 6, 12} <= joints


def test_the_autograd_function_asks_only_for_what_backward_reads_and_refuses_a_second_derivative():
    """forward_dynamics_fn on a stand-in that records `want`: the matrices of the inputs that need no gradient are neither asked for
    nor saved, backward is g^T J, and a gradient of a gradient raises (backward is once_differentiable) instead of returning zero."""
    import torch
    from diy_gym_amd.backend import DynamicsDerivatives, HipBackend

    class StandIn:
        def forward_dynamics_derivatives(self, body, q, qd, tau, joint_damping, want):
            self.want = want
            B, n = q.shape
            m = lambda k: (torch.arange(n * n, dtype=torch.float32).reshape(n, n) * k).expand(B, n, n).contiguous()
            return DynamicsDerivatives(q + tau, m(1.0) if 'dqdd_dq' in want else None, m(2.0) if 'dqdd_dqd' in want else None, m(3.0) if 'dqdd_dtau' in want else None,
                                       None, None, None)
    sim = StandIn()
    f = HipBackend.forward_dynamics_fn(sim, 0)
    q, qd, tau = torch.ones(2, 3), torch.ones(2, 3), torch.ones(2, 3, requires_grad=True)
    f(q, qd, tau).sum().backward()
    assert sim.want == ('qdd', 'dqdd_dtau') and tau.grad.tolist() == [[27.0, 36.0, 45.0]] * 2   # the column sums of 3 x [[0 1 2] [3 4 5] [6 7 8]]
    q.requires_grad_(True)
    f(q, qd, tau).sum().backward()
    assert sim.want == ('qdd', 'dqdd_dq', 'dqdd_dtau') and q.grad.tolist() == [[9.0, 12.0, 15.0]] * 2 and qd.grad is None
    g, = torch.autograd.grad(f(q, qd, tau).sum(), tau, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()

"""What the ``dg_world_*`` entries refuse, and in which words: every refusal the entries share through a helper of
diy_gym_amd/csrc/dg_api.hip (body range, frame lookup, impulse cache, the dynamics queries' body checks) and the entry's own
refusals around them, called through ``env.sim.lib`` with raw ctypes.  Each call pins the return code and the WHOLE
``dg_last_error()`` string, written out here as the source had it before the helpers were shared; the doubly-wrong calls pin which
message wins.  Nothing is launched by a refused call, and the state keeps its bits.

One world of 2 envs: tests/golden/joint_wrench/pendulum_prop.yaml (``prop``: frozen static body 0; ``pend``: fixed base, one
joint, two frames, saved velocities, body 1) with the floating cart of cart_tree.urdf (body 2: joints, no saved velocities) and a
free box (body 3: no joints) added beside it; and the same world without the contact impulse cache.

Not reachable from a world the planner accepts, so not pinned here: "needs %d workspace slots" (the planner gives every body the
slots its queries need: tests/test_dynamics_cabi.py, tests/test_ik_cabi.py), the grid-limit refusals, a fixed base without joints
that is not frozen, and the refusals that need a respawn addon or a frame on the base of a body with saved velocities."""
import ctypes
import os

import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
pytestmark = pytest.mark.gpu

OK, UNSUPPORTED, ARG = 0, -3, -4   # DG_OK, DG_ERR_UNSUPPORTED, DG_ERR_ARG
ANY = -2                           # DG_CONTACT_ANY
PROP, PEND, CART, BOX = 0, 1, 2, 3
B = 2


def make(**kw):
    from diy_gym_amd import DIYGym
    from diy_gym_amd.config import Configuration
    cfg = os.path.join(GOLDEN, 'joint_wrench', 'pendulum_prop.yaml')
    tree = yaml.safe_load(open(cfg))
    tree['cart'] = {'model': '../urdf/cart_tree.urdf', 'xyz': [2.0, 0.0, 0.45]}
    tree['box'] = {'model': '../urdf/box_upper.urdf', 'xyz': [-2.0, 0.0, 0.3]}
    conf = Configuration.from_dict('entry_refusals', tree)
    conf.source_dir = os.path.dirname(cfg)
    return DIYGym(conf, num_envs=B, seed=5, device='cuda:0', **kw)


class World:
    """A world, buffers any entry can be handed, and ``refuse``: one call, its code and its words."""
    def __init__(self, env):
        import torch
        self.env, self.sim, self.lib = env, env.sim, env.sim.lib
        self.f = torch.zeros(1 << 20, dtype=torch.float32, device=env.device)   # any float output or input
        self.i = torch.zeros(1 << 20, dtype=torch.int32, device=env.device)     # any int32 output
        self.S, self.F, self.I = (ctypes.c_void_p(t.data_ptr()) for t in (self.sim.state, self.f, self.i))

    def call(self, entry, *args):
        return getattr(self.lib, 'dg_world_' + entry)(self.sim.handle, *args, self.sim._stream())

    def refuse(self, code, text, entry, *args):
        rc = self.call(entry, *args)
        assert (rc, self.lib.dg_last_error().decode()) == (code, text), entry


@pytest.fixture(scope='module')
def worlds():
    env = make()
    bare = make(engine={'warmstart': 0, 'warmstart_friction': 0})
    for e in (env, bare):
        assert [e.models[k].uid for k in ('prop', 'pend', 'cart', 'box')] == [PROP, PEND, CART, BOX]
    assert env.layout.warm_off >= 0 and bare.layout.warm_off < 0 and bare.layout.max_contacts > 0
    assert len(env.models['pend'].flat.frames) == 2 and len(env.models['pend'].flat.links) == 1
    return World(env), World(bare)


@pytest.fixture
def w(worlds):
    """The world with the impulse cache; the state's bits of both worlds are the same after the test as before it."""
    import torch
    before = [x.sim.state.clone() for x in worlds]
    yield worlds[0]
    torch.cuda.synchronize()
    for x, s in zip(worlds, before):
        assert torch.equal(x.sim.state.view(torch.int32), s.view(torch.int32))


@pytest.fixture
def bare(worlds, w):
    return worlds[1]


def i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def test_raycast(w):
    S, F, I = w.S, w.F, w.I

    def ray(code, text, state=S, body=PEND, frame=0, n=1, skip=-1, scratch=F, frac=F):
        w.refuse(code, text, 'raycast', state, body, frame, n, F, F, 0, skip, scratch, frac, I, F, F)
    ray(ARG, 'null argument', state=None)
    ray(ARG, 'n_rays must be positive, got 0', n=0)
    ray(ARG, 'frac is NULL (id, pos and normal may be)', frac=None)
    ray(ARG, 'scratch is NULL (dg_world_raycast_scratch_floats floats of device memory)', scratch=None)
    ray(ARG, 'body 4 out of range', body=4)
    ray(ARG, 'body -2 out of range', body=-2)
    ray(ARG, 'skip_body 9 out of range', skip=9)
    ray(ARG, 'frame 0 given without a body', body=-1)
    ray(ARG, 'frame -2 out of range', frame=-2)
    ray(ARG, 'body 1 has no frame 2', frame=2)
    # doubly wrong: the earlier check's words
    ray(ARG, 'body 4 out of range', body=4, frame=7)
    ray(ARG, 'skip_body 9 out of range', skip=9, frame=7)
    ray(ARG, 'frac is NULL (id, pos and normal may be)', frac=None, frame=7)


def test_frame_state(w):
    S, F = w.S, w.F
    w.refuse(ARG, 'null argument', 'frame_state', None, PEND, 0, 0, F)
    w.refuse(ARG, 'null argument', 'frame_state', S, 4, 0, 0, None)
    w.refuse(ARG, 'body -1 out of range', 'frame_state', S, -1, 0, 0, F)
    w.refuse(ARG, 'body 4 out of range', 'frame_state', S, 4, 0, 0, F)
    w.refuse(ARG, 'body 1 has no frame 2', 'frame_state', S, PEND, 2, 0, F)
    w.refuse(ARG, 'body 3 has no frame 0', 'frame_state', S, BOX, 0, 0, F)
    w.refuse(ARG, 'body 4 out of range', 'frame_state', S, 4, 9, 0, F)   # doubly wrong
    assert w.call('frame_state', S, PEND, 1, 0, F) == OK and w.call('frame_state', S, CART, -1, 1, F) == OK


def test_apply_wrench(w):
    S, F = w.S, w.F
    w.refuse(ARG, 'null argument', 'apply_wrench', None, PEND, 0, 2, F, F, F)
    w.refuse(ARG, 'body 4 out of range', 'apply_wrench', S, 4, 0, 2, F, F, F)
    w.refuse(ARG, 'body 0 is part of the frozen static world: it has no state to push on', 'apply_wrench', S, PROP, -1, 2, F, F, F)
    w.refuse(ARG, 'flags must be DG_WRENCH_LINK_FRAME (1) or DG_WRENCH_WORLD_FRAME (2)', 'apply_wrench', S, PEND, 0, 3, F, F, F)
    w.refuse(ARG, 'body 1 has no frame 2', 'apply_wrench', S, PEND, 2, 1, F, F, F)
    # doubly wrong
    w.refuse(ARG, 'body -1 out of range', 'apply_wrench', S, -1, 2, 0, F, F, F)
    w.refuse(ARG, 'body 0 is part of the frozen static world: it has no state to push on', 'apply_wrench', S, PROP, 5, 0, F, F, F)
    w.refuse(ARG, 'flags must be DG_WRENCH_LINK_FRAME (1) or DG_WRENCH_WORLD_FRAME (2)', 'apply_wrench', S, PEND, 2, 0, F, F, F)
    w.refuse(ARG, 'body 1 has no frame 2', 'apply_wrench', S, PEND, 2, 1, None, None, None)   # before the early DG_OK
    assert w.call('apply_wrench', S, PEND, 0, 1, None, F, None) == OK   # no force, no torque: nothing to do


def test_dynamics_queries(w):
    S, F = w.S, w.F
    lp = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    # the body checks the eight entries share, under each entry's name
    w.refuse(ARG, 'dg_world_joint_state: null argument', 'joint_state', None, PEND, F, F)
    w.refuse(ARG, 'dg_world_joint_state: body 4 out of range', 'joint_state', S, 4, F, F)
    w.refuse(ARG, 'dg_world_joint_state: body -1 out of range', 'joint_state', S, -1, F, F)
    w.refuse(ARG, 'dg_world_joint_state: body 0 is part of the frozen static world: it has no joints', 'joint_state', S, PROP, F, F)
    w.refuse(ARG, 'dg_world_joint_state: body 2 has a floating base; the dynamics queries take fixed-base bodies only', 'joint_state', S, CART, F, F)
    w.refuse(ARG, 'dg_world_joint_state: body 3 has a floating base; the dynamics queries take fixed-base bodies only', 'joint_state', S, BOX, F, F)
    w.refuse(ARG, 'dg_world_joint_state: body 4 out of range', 'joint_state', S, 4, None, None)   # before the early DG_OK
    assert w.call('joint_state', S, PEND, None, None) == OK
    w.refuse(ARG, 'dg_world_jacobian: body 4 out of range', 'jacobian', S, 4, 0, lp, None, F, F)
    w.refuse(ARG, 'dg_world_jacobian: local_pos is NULL (three host floats)', 'jacobian', S, PEND, 0, None, None, F, F)
    w.refuse(ARG, 'dg_world_jacobian: frame -1 out of range (the base of a fixed body does not move)', 'jacobian', S, PEND, -1, lp, None, F, F)
    w.refuse(ARG, 'dg_world_jacobian: body 1 has no frame 2', 'jacobian', S, PEND, 2, lp, None, F, F)
    w.refuse(ARG, 'dg_world_jacobian: body 2 has a floating base; the dynamics queries take fixed-base bodies only', 'jacobian', S, CART, 9, None, None, F, F)
    w.refuse(ARG, 'dg_world_jacobian: local_pos is NULL (three host floats)', 'jacobian', S, PEND, 2, None, None, F, F)
    w.refuse(ARG, 'dg_world_jacobian: body 1 has no frame 2', 'jacobian', S, PEND, 2, lp, None, None, None)   # before the early DG_OK
    assert w.call('jacobian', S, PEND, 1, lp, None, None, None) == OK
    w.refuse(ARG, 'dg_world_inverse_dynamics: body 4 out of range', 'inverse_dynamics', S, 4, None, None, None, F)
    w.refuse(ARG, 'dg_world_inverse_dynamics: tau is NULL', 'inverse_dynamics', S, PEND, None, None, None, None)
    w.refuse(ARG, 'dg_world_inverse_dynamics: body 0 is part of the frozen static world: it has no joints', 'inverse_dynamics', S, PROP, None, None, None, None)
    w.refuse(ARG, 'dg_world_mass_matrix: null argument', 'mass_matrix', None, PEND, None, F)
    w.refuse(ARG, 'dg_world_mass_matrix: body -1 out of range', 'mass_matrix', S, -1, None, F)
    w.refuse(ARG, 'dg_world_mass_matrix: M is NULL', 'mass_matrix', S, PEND, None, None)
    w.refuse(ARG, 'dg_world_apply_joint_torque: body 0 is part of the frozen static world: it has no joints', 'apply_joint_torque', S, PROP, F)
    w.refuse(ARG, 'dg_world_apply_joint_torque: tau is NULL', 'apply_joint_torque', S, PEND, None)


def test_inverse_kinematics_targets_and_joint_reset(w):
    S, F, I = w.S, w.F, w.I

    def ik(text, body=PEND, frame=1, pos=F, q_out=F):
        w.refuse(ARG, text, 'inverse_kinematics', S, body, frame, pos, None, None, None, q_out, I)
    ik('dg_world_inverse_kinematics: body 4 out of range', body=4)
    ik('dg_world_inverse_kinematics: body 2 has a floating base; the dynamics queries take fixed-base bodies only', body=CART)
    ik('dg_world_inverse_kinematics: frame -1 out of range (the base of a fixed body does not move)', frame=-1)
    ik('dg_world_inverse_kinematics: body 1 has no frame 2', frame=2)
    ik('dg_world_inverse_kinematics: target_pos is NULL', pos=None)
    ik('dg_world_inverse_kinematics: q_out is NULL', q_out=None)
    ik('dg_world_inverse_kinematics: body 1 has no frame 2', frame=2, pos=None, q_out=None)   # doubly wrong
    ik('dg_world_inverse_kinematics: target_pos is NULL', pos=None, q_out=None)
    w.refuse(ARG, 'dg_world_set_joint_targets: body 4 out of range', 'set_joint_targets', S, 4, ctypes.c_uint64(1), F, F)
    w.refuse(ARG, 'dg_world_set_joint_targets: pos and vel are both NULL', 'set_joint_targets', S, PEND, ctypes.c_uint64(1), None, None)
    w.refuse(ARG, 'dg_world_reset_joint_state: body 2 has a floating base; the dynamics queries take fixed-base bodies only', 'reset_joint_state',
             S, CART, ctypes.c_uint64(1), F, None, None)
    w.refuse(ARG, 'dg_world_reset_joint_state: q is NULL', 'reset_joint_state', S, PEND, ctypes.c_uint64(1), None, None, None)


def test_link_states_and_base_reset(w):
    S, F = w.S, w.F
    w.refuse(ARG, 'dg_world_link_states: null argument', 'link_states', None, i32(PEND), i32(0), 1, 0, F)
    w.refuse(ARG, 'dg_world_link_states: bodies, frames or out is NULL', 'link_states', S, i32(PEND), i32(0), 1, 0, None)
    w.refuse(ARG, 'dg_world_link_states: bodies, frames or out is NULL', 'link_states', S, None, i32(0), 0, 0, F)
    w.refuse(ARG, 'dg_world_link_states: n must be 1 .. 32, got 0', 'link_states', S, i32(4), i32(0), 0, 0, F)
    w.refuse(ARG, 'dg_world_link_states: n must be 1 .. 32, got 33', 'link_states', S, i32(*[PEND] * 33), i32(*[0] * 33), 33, 0, F)
    w.refuse(ARG, 'dg_world_link_states: bodies[1] = 4 out of range', 'link_states', S, i32(PEND, 4), i32(0, 0), 2, 0, F)
    w.refuse(ARG, 'dg_world_link_states: bodies[0] = -1 out of range', 'link_states', S, i32(-1, PEND), i32(0, 7), 2, 0, F)
    w.refuse(ARG, 'dg_world_link_states: body 2 has no frame 9 (selector 1)', 'link_states', S, i32(PEND, CART), i32(-1, 9), 2, 0, F)
    w.refuse(ARG, 'dg_world_link_states: body 1 has no frame 7 (selector 0)', 'link_states', S, i32(PEND, 4), i32(7, 0), 2, 0, F)   # the first selector's
    assert w.call('link_states', S, i32(BOX, PEND, CART), i32(-1, 1, -5), 3, 1, F) == OK
    w.refuse(ARG, 'dg_world_reset_base_state: null argument', 'reset_base_state', None, CART, F, F, F, F, None)
    w.refuse(ARG, 'dg_world_reset_base_state: body 4 out of range', 'reset_base_state', S, 4, F, F, F, F, None)
    w.refuse(ARG, 'dg_world_reset_base_state: pos and orn go together (both or neither)', 'reset_base_state', S, CART, F, None, F, F, None)
    w.refuse(ARG, 'dg_world_reset_base_state: nothing to write (pos, orn, lin_vel and ang_vel are all NULL)', 'reset_base_state', S, CART, None, None, None, None, None)
    pinned = ('dg_world_reset_base_state: body %d has a fixed base that the scene pins to its load pose; add a respawn addon to the model '
              '(zero ranges will do) to make its base movable')
    w.refuse(ARG, pinned % PEND, 'reset_base_state', S, PEND, F, F, None, None, None)
    w.refuse(ARG, pinned % PROP, 'reset_base_state', S, PROP, None, None, F, None, None)
    w.refuse(ARG, 'dg_world_reset_base_state: body -1 out of range', 'reset_base_state', S, -1, F, None, None, None, None)   # doubly wrong
    w.refuse(ARG, 'dg_world_reset_base_state: pos and orn go together (both or neither)', 'reset_base_state', S, PEND, None, F, None, None, None)


NO_CACHE = ('%s: the world keeps no contact impulse cache (warmstart and warmstart_friction are 0, or the scene has no candidate pairs): '
            'no forces to report')


def test_contacts_and_contact_forces(w, bare):
    S, F, I = w.S, w.F, w.I
    for x in (w, bare):   # the argument checks come first in either world
        x.refuse(ARG, 'dg_world_contacts: null argument', 'contacts', None, ANY, ANY, ANY, ANY, x.I, x.I, x.F, x.F)
        x.refuse(ARG, 'dg_world_contacts: count is NULL (ids, geom and force may be)', 'contacts', x.S, 4, ANY, ANY, ANY, None, x.I, x.F, x.F)
        x.refuse(ARG, 'dg_world_contacts: link_a 0 given without body_a', 'contacts', x.S, ANY, 0, 4, ANY, x.I, x.I, x.F, x.F)
        x.refuse(ARG, 'dg_world_contacts: body_a 4 out of range', 'contacts', x.S, 4, ANY, -1, ANY, x.I, x.I, x.F, x.F)
        x.refuse(ARG, 'dg_world_contacts: body_b -1 out of range', 'contacts', x.S, PEND, ANY, -1, ANY, x.I, x.I, x.F, x.F)
        x.refuse(ARG, 'dg_world_contacts: body 1 has no link 7', 'contacts', x.S, PEND, 7, ANY, ANY, x.I, x.I, x.F, x.F)
        x.refuse(ARG, 'dg_world_contacts: body 2 has no link -3', 'contacts', x.S, PEND, 1, CART, -3, x.I, x.I, x.F, x.F)
        x.refuse(ARG, 'dg_world_contact_forces: null argument', 'contact_forces', None, ANY, ANY, ANY, ANY, x.I, x.I, x.F)
        x.refuse(ARG, 'dg_world_contact_forces: count is NULL (ids and forces may be)', 'contact_forces', x.S, ANY, ANY, ANY, ANY, None, x.I, x.F)
        x.refuse(ARG, 'dg_world_contact_forces: link_b 1 given without body_b', 'contact_forces', x.S, PEND, ANY, ANY, 1, x.I, x.I, x.F)
        x.refuse(ARG, 'dg_world_contact_forces: body_a 9 out of range', 'contact_forces', x.S, 9, ANY, ANY, 1, x.I, x.I, x.F)
        x.refuse(ARG, 'dg_world_contact_forces: body 1 has no link 7', 'contact_forces', x.S, PEND, 7, ANY, ANY, x.I, x.I, x.F)
    bare.refuse(UNSUPPORTED, NO_CACHE % 'dg_world_contacts', 'contacts', bare.S, PEND, ANY, ANY, ANY, bare.I, bare.I, bare.F, bare.F)
    assert bare.call('contacts', bare.S, PEND, ANY, ANY, ANY, bare.I, bare.I, bare.F, None) == OK   # no forces asked for
    bare.refuse(UNSUPPORTED, NO_CACHE % 'dg_world_contact_forces', 'contact_forces', bare.S, ANY, ANY, ANY, ANY, bare.I, None, None)
    assert w.call('contacts', S, PEND, ANY, ANY, ANY, I, I, F, F) == OK


def test_net_contact_wrench(w, bare):
    for x in (w, bare):
        S, F, I = x.S, x.F, x.I
        x.refuse(ARG, 'dg_world_net_contact_wrench: null argument', 'net_contact_wrench', None, PEND, i32(ANY), 1, ANY, ANY, F, I)
        x.refuse(ARG, 'dg_world_net_contact_wrench: links or wrench is NULL (ncontacts may be)', 'net_contact_wrench', S, 4, i32(ANY), 0, ANY, ANY, None, I)
        x.refuse(ARG, 'dg_world_net_contact_wrench: n must be 1 .. 16, got 0', 'net_contact_wrench', S, 4, i32(ANY), 0, ANY, ANY, F, I)
        x.refuse(ARG, 'dg_world_net_contact_wrench: n must be 1 .. 16, got 17', 'net_contact_wrench', S, PEND, i32(*[ANY] * 17), 17, ANY, ANY, F, I)
        x.refuse(ARG, 'dg_world_net_contact_wrench: body 4 out of range', 'net_contact_wrench', S, 4, i32(5), 1, 4, ANY, F, I)
        x.refuse(ARG, 'dg_world_net_contact_wrench: body -2 out of range', 'net_contact_wrench', S, ANY, i32(ANY), 1, ANY, ANY, F, I)
        x.refuse(ARG, 'dg_world_net_contact_wrench: links[1] = 2 is not a frame of body 1 (DG_CONTACT_ANY: the whole body)', 'net_contact_wrench',
                 S, PEND, i32(-1, 2), 2, 4, ANY, F, I)
        x.refuse(ARG, 'dg_world_net_contact_wrench: links[0] = -3 is not a frame of body 1 (DG_CONTACT_ANY: the whole body)', 'net_contact_wrench',
                 S, PEND, i32(-3), 1, ANY, ANY, F, I)
        x.refuse(ARG, 'dg_world_net_contact_wrench: body_b 4 out of range', 'net_contact_wrench', S, PEND, i32(ANY, 0, 1), 3, 4, ANY, F, I)
        x.refuse(ARG, 'dg_world_net_contact_wrench: link_b 0 given without body_b', 'net_contact_wrench', S, PEND, i32(ANY), 1, ANY, 0, F, I)
    bare.refuse(UNSUPPORTED, NO_CACHE % 'dg_world_net_contact_wrench', 'net_contact_wrench', bare.S, PEND, i32(ANY), 1, ANY, ANY, bare.F, None)
    assert w.call('net_contact_wrench', w.S, PEND, i32(ANY, -1, 1), 3, PROP, ANY, w.F, None) == OK


def test_joint_wrench_and_efforts(w, bare):
    from diy_gym_amd.backend import JointSelector
    no_prev = ('dg_world_joint_wrench: body %d keeps no saved velocities; call builder.enable_joint_force_torque(body) while the scene is built '
               '(joint_wrench_sensor does), or put a compiled force_torque_sensor on the body')

    def sel(frame=0, flags=0, link_mask=1, frame_mask=1):
        a = (JointSelector * 1)()
        a[0].frame, a[0].flags, a[0].link_mask, a[0].frame_mask = frame, flags, link_mask, frame_mask
        return a
    for x in (w, bare):
        S, F = x.S, x.F
        x.refuse(ARG, 'dg_world_joint_wrench: null argument', 'joint_wrench', None, PEND, sel(), 1, F)
        x.refuse(ARG, 'dg_world_joint_wrench: selectors or wrench is NULL', 'joint_wrench', S, 4, None, 0, F)
        x.refuse(ARG, 'dg_world_joint_wrench: selectors or wrench is NULL', 'joint_wrench', S, PEND, sel(), 1, None)
        x.refuse(ARG, 'dg_world_joint_wrench: n must be 1 .. 16, got 0', 'joint_wrench', S, 4, sel(), 0, F)
        x.refuse(ARG, 'dg_world_joint_wrench: n must be 1 .. 16, got 17', 'joint_wrench', S, PEND, sel(), 17, F)
        x.refuse(ARG, 'dg_world_joint_wrench: body 4 out of range', 'joint_wrench', S, 4, sel(frame=9), 1, F)
        x.refuse(ARG, 'dg_world_joint_wrench: body -1 out of range', 'joint_wrench', S, -1, sel(), 1, F)
        x.refuse(ARG, 'dg_world_joint_wrench: body 0 is part of the frozen static world: it has no joints', 'joint_wrench', S, PROP, sel(), 1, F)
        x.refuse(ARG, no_prev % CART, 'joint_wrench', S, CART, sel(frame=9), 1, F)
        x.refuse(ARG, no_prev % BOX, 'joint_wrench', S, BOX, sel(), 1, F)
        x.refuse(ARG, 'dg_world_joint_wrench: body 1 has no frame 2 (selector 0)', 'joint_wrench', S, PEND, sel(frame=2, link_mask=2), 1, F)
        x.refuse(ARG, 'dg_world_joint_wrench: body 1 has no frame -1 (selector 0)', 'joint_wrench', S, PEND, sel(frame=-1), 1, F)
        x.refuse(ARG, "dg_world_joint_wrench: selector 0 names a link or frame past the body's 1 links and 2 frames", 'joint_wrench', S, PEND, sel(link_mask=2), 1, F)
        x.refuse(ARG, "dg_world_joint_wrench: selector 0 names a link or frame past the body's 1 links and 2 frames", 'joint_wrench', S, PEND, sel(frame_mask=4), 1, F)
        x.refuse(ARG, 'dg_world_joint_efforts: null argument', 'joint_efforts', S, 4, None)
        x.refuse(ARG, 'dg_world_joint_efforts: body 4 out of range', 'joint_efforts', S, 4, F)
        x.refuse(ARG, 'dg_world_joint_efforts: body 0 is part of the frozen static world: it has no joints', 'joint_efforts', S, PROP, F)
        x.refuse(ARG, 'dg_world_joint_efforts: body 3 has no joints', 'joint_efforts', S, BOX, F)
        assert x.call('joint_efforts', S, CART, F) == OK
    bare.refuse(UNSUPPORTED, 'dg_world_joint_wrench: the world keeps no contact impulse cache (warmstart and warmstart_friction are 0): no contact forces '
                'to take off the child side', 'joint_wrench', bare.S, PEND, sel(), 1, bare.F)
    from diy_gym_amd.backend import joint_wrench_selectors
    assert w.call('joint_wrench', w.S, PEND, joint_wrench_selectors(w.env.layout, PEND, [1])[2], 1, w.F) == OK


def test_link_accelerations(w):
    from diy_gym_amd.backend import AccelSelector
    S, F = w.S, w.F

    def sel(frame=0, quat=(0.0, 0.0, 0.0, 2.0)):
        a = (AccelSelector * 1)()
        a[0].frame = frame; a[0].quat[:] = quat
        return a
    w.refuse(ARG, 'dg_world_link_accelerations: null argument', 'link_accelerations', None, PEND, sel(), 1, F)
    w.refuse(ARG, 'dg_world_link_accelerations: selectors or out is NULL', 'link_accelerations', S, 4, sel(), 0, None)
    w.refuse(ARG, 'dg_world_link_accelerations: n must be 1 .. 16, got 17', 'link_accelerations', S, 4, sel(), 17, F)
    w.refuse(ARG, 'dg_world_link_accelerations: n must be 1 .. 16, got 0', 'link_accelerations', S, PEND, sel(), 0, F)
    w.refuse(ARG, 'dg_world_link_accelerations: body 4 out of range', 'link_accelerations', S, 4, sel(frame=5), 1, F)
    w.refuse(ARG, 'dg_world_link_accelerations: body 0 is part of the frozen static world: it never moves', 'link_accelerations', S, PROP, sel(), 1, F)
    w.refuse(ARG, 'dg_world_link_accelerations: body 2 keeps no saved velocities; call builder.enable_joint_force_torque(body) while the scene is built '
             '(imu_sensor does), or put a compiled force_torque_sensor on the body; a fixed base without joints keeps none', 'link_accelerations',
             S, CART, sel(frame=9), 1, F)
    w.refuse(ARG, 'dg_world_link_accelerations: body 1 has no frame 2 (selector 0)', 'link_accelerations', S, PEND, sel(frame=2), 1, F)
    w.refuse(ARG, 'dg_world_link_accelerations: body 1 has no frame -2 (selector 0)', 'link_accelerations', S, PEND, sel(frame=-2), 1, F)
    w.refuse(ARG, 'dg_world_link_accelerations: the mount quaternion of selector 0 has zero norm', 'link_accelerations', S, PEND, sel(quat=(0.0, ) * 4), 1, F)
    w.refuse(ARG, 'dg_world_link_accelerations: body 1 has no frame 2 (selector 0)', 'link_accelerations', S, PEND, sel(frame=2, quat=(0.0, ) * 4), 1, F)
    assert w.call('link_accelerations', S, PEND, sel(frame=-1), 1, F) == OK

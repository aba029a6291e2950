"""ctypes binding of the C-ABI in ``include/diygym_hip.h`` (``libdiygym_hip.so``).

This is the only compute path of the package.  There is no CPU fallback: if the
HIP library has not been built, or no GPU is visible, constructing a backend
raises.  (The CPU oracle under ``oracle/`` is test infrastructure and is never
imported from here.)
"""
import collections
import ctypes
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libdiygym_hip.so')

_lib = None

_c_i32p = ctypes.POINTER(ctypes.c_int32)
_c_f64p = ctypes.POINTER(ctypes.c_double)
_vp = ctypes.c_void_p


class JointSelector(ctypes.Structure):
    """``dg_joint_selector`` of include/diygym_hip.h: one joint of ``dg_world_joint_wrench``."""
    _fields_ = [('frame', ctypes.c_int32), ('flags', ctypes.c_int32), ('link_mask', ctypes.c_uint64), ('frame_mask', ctypes.c_uint64),
                ('rigid', ctypes.c_float * 10)]


class AccelSelector(ctypes.Structure):
    """``dg_accel_selector`` of include/diygym_hip.h: one sensor frame of ``dg_world_link_accelerations``."""
    _fields_ = [('frame', ctypes.c_int32), ('com', ctypes.c_int32), ('pos', ctypes.c_float * 3), ('quat', ctypes.c_float * 4)]


# every symbol include/diygym_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'dg_version': (ctypes.c_int32, []),
    'dg_last_error': (ctypes.c_char_p, []),
    'dg_world_create': (ctypes.c_int32, [_c_i32p, ctypes.c_int64, _c_f64p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64, ctypes.POINTER(_vp)]),
    'dg_world_destroy': (None, [_vp]),
    'dg_world_dims': (ctypes.c_int32, [_vp, _c_i32p]),
    'dg_world_kernel_name': (ctypes.c_char_p, [_vp]),
    'dg_world_get_motor_cfg': (ctypes.c_int32, [_vp, _c_f64p]),
    'dg_world_set_motor_cfg': (ctypes.c_int32, [_vp, _c_f64p]),
    'dg_world_init_state': (ctypes.c_int32, [_vp, _vp, _vp]),
    'dg_world_reset': (ctypes.c_int32, [_vp, _vp, _vp, _vp, _vp]),
    'dg_world_step': (ctypes.c_int32, [_vp, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_observe': (ctypes.c_int32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_frame_state': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp]),
    'dg_world_apply_wrench': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp]),
    'dg_world_render': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp]),
    'dg_world_raycast_scratch_floats': (ctypes.c_int64, [_vp]),
    'dg_world_raycast': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp,
                                          _vp, _vp, _vp, _vp, _vp]),
    'dg_world_joint_state': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, _vp, _vp, _vp]),
    'dg_world_jacobian': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_float), _vp, _vp, _vp, _vp]),
    'dg_world_inverse_dynamics': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_mass_matrix': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, _vp, _vp, _vp]),
    'dg_world_apply_joint_torque': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, _vp, _vp]),
    'dg_world_inverse_kinematics': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_set_joint_targets': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_uint64, _vp, _vp, _vp]),
    'dg_world_reset_joint_state': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_uint64, _vp, _vp, _vp, _vp]),
    'dg_world_contacts': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_contact_forces': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp]),
    'dg_world_net_contact_wrench': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, _c_i32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp]),
    'dg_world_link_states': (ctypes.c_int32, [_vp, _vp, _c_i32p, _c_i32p, ctypes.c_int32, ctypes.c_int32, _vp, _vp]),
    'dg_world_reset_base_state': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_joint_wrench': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.POINTER(JointSelector), ctypes.c_int32, _vp, _vp]),
    'dg_world_joint_efforts': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, _vp, _vp]),
    'dg_world_link_accelerations': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.POINTER(AccelSelector), ctypes.c_int32, _vp, _vp]),
    'dg_world_task_space': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_float), ctypes.c_int32, _vp, _vp, _vp, _vp,
                                             ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_forward_dynamics': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp]),
    'dg_world_rollout': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_float), ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                          ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_dynamics_derivatives': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_rollout_feedback': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_float), ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                                   ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_inertial_parameters': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp, _vp]),
    'dg_world_id_regressor': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_lq_backward': (ctypes.c_int32, [_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_closest_scratch_floats': (ctypes.c_int64, [_vp]),
    'dg_world_closest': (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_int32, _vp,
                                          _vp, _vp, _vp, _vp, _vp, _vp]),
    'dg_world_set_render_diag': (ctypes.c_int32, [_vp, ctypes.c_int32]),
    'dg_world_set_diag_buffer': (ctypes.c_int32, [_vp, _vp]),
    'dg_world_set_skip_counter': (ctypes.c_int32, [_vp, _vp]),
    'dg_world_set_profile_buffer': (ctypes.c_int32, [_vp, _vp]),
    'dg_debug_plan': (ctypes.c_int32, [_c_i32p, ctypes.c_int64, _c_f64p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _c_i32p, _c_i32p,
                                       ctypes.c_int64]),
}


def load_library(path=None):
    """Load ``libdiygym_hip.so`` and type every exported entry point."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.isfile(path):
        raise RuntimeError('HIP library not built: %s is missing. Run `python -c "import __graft_entry__ as g; g.build()"` '
                           '(or `make -j8 -C diy_gym_amd/csrc`).  There is no CPU fallback.' % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _scene_constants():
    from .scene import K
    return K


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# what ray_test_batch returns: device tensors, None for the outputs `want` left out
RayHits = collections.namedtuple('RayHits', ['frac', 'id', 'pos', 'normal'])

# what contact_points returns: device tensors, None for the outputs `want` left out (count is always there)
ContactPoints = collections.namedtuple('ContactPoints', ['count', 'id_a', 'id_b', 'pos_a', 'pos_b', 'normal', 'distance', 'normal_force'])
CONTACT_ANY = -2   # DG_CONTACT_ANY

# what contact_forces returns: device tensors, None for the outputs `want` left out (count is always there)
ContactForces = collections.namedtuple('ContactForces', ['count', 'id_a', 'id_b', 'normal', 'normal_force', 'lateral_friction1', 'lateral_dir1',
                                                         'lateral_friction2', 'lateral_dir2', 'force_on_a'])
CONTACT_MAX_LINKS = 16   # DG_CONTACT_MAX_LINKS: link selectors of one net_contact_forces call

# what closest_points returns: device tensors, None for the outputs `want` left out (count is always there)
ClosestPoints = collections.namedtuple('ClosestPoints', ['count', 'id_a', 'id_b', 'pos_a', 'pos_b', 'normal', 'distance', 'nearest_id_a', 'nearest_id_b',
                                                         'nearest_pos_a', 'nearest_pos_b', 'nearest_normal', 'nearest_distance'])
CLOSEST_MAX_POINTS = 64   # the cap of closest_points' default K
LINK_STATES_MAX = 32   # DG_LINK_STATES_MAX: (body, frame) selectors of one link_states call
JOINT_WRENCH_MAX = 16   # DG_JOINT_WRENCH_MAX: joint selectors of one joint_reaction_forces call
# what task_space_dynamics returns: device tensors, None for the outputs `want` left out.  `lambda` is a Python keyword: the field
# is `lambda_` (`want` takes either spelling)
TaskSpaceDynamics = collections.namedtuple('TaskSpaceDynamics', ['jac', 'bias_acc', 'bias_torque', 'lambda_', 'tau', 'point', 'singular'])
# what rollout_joint_dynamics returns: device tensors, None for the outputs `want` left out
JointRollout = collections.namedtuple('JointRollout', ['q', 'qd', 'pos', 'singular'])
# what forward_dynamics_derivatives returns: device tensors, None for the outputs `want` left out
DynamicsDerivatives = collections.namedtuple('DynamicsDerivatives', ['qdd', 'dqdd_dq', 'dqdd_dqd', 'dqdd_dtau', 'dtau_dq', 'dtau_dqd', 'singular'])
# what inverse_dynamics_regressor returns: device tensors, None for the outputs `want` left out
DynamicsRegressor = collections.namedtuple('DynamicsRegressor', ['Y', 'tau', 'grad'])
# what rollout_joint_feedback returns: device tensors, None for the outputs `want` left out
FeedbackRollout = collections.namedtuple('FeedbackRollout', ['q', 'qd', 'tau', 'pos', 'singular'])
# what lq_backward_pass returns: device tensors, None for the outputs `want` left out (status is always there)
LqBackward = collections.namedtuple('LqBackward', ['K', 'k', 'dV', 'status'])
LINK_ACCEL_MAX = 16   # DG_LINK_ACCEL_MAX: sensor-frame selectors of one link_accelerations call
# what link_accelerations returns: [B, n, 3] views of ONE [B, n, 15] buffer, at the columns DG_LA_* of include/diygym_hip.h
LinkAccelerations = collections.namedtuple('LinkAccelerations', ['lin_acc', 'ang_acc', 'specific_force', 'ang_vel', 'gravity'])
LA_LIN_ACC, LA_ANG_ACC, LA_SPECIFIC_FORCE, LA_ANG_VEL, LA_GRAVITY, LA_STRIDE = 0, 3, 6, 9, 12, 15


def _mount_key(v):
    """A hashable stand-in for a mount argument of ``link_accelerations``: None, one vector or n rows; lists, arrays or tensors."""
    if v is None:
        return None
    if isinstance(v, (list, tuple)) and all(isinstance(x, (int, float)) for x in v):
        return tuple(v)   # (one vector as a plain list: what imu_sensor passes every tick)
    return tuple(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64).ravel().tolist())


def link_accel_selectors(layout, body, frames=None, local_pos=None, local_orn=None, com=False):
    """The selectors ``dg_world_link_accelerations`` takes for sensor frames of ``body`` (a Model's ``uid``), from the scene alone:
    ``(body index, (AccelSelector * n))``.  ``frames``: what ``Model.get_frame_id`` returns, -1 the base (None: the base alone);
    ``local_pos`` ``[n, 3]`` and ``local_orn`` ``[n, 4]`` xyzw the mount in that frame (one vector: every selector; None: identity).
    ValueError for what the entry would refuse."""
    K = _scene_constants()
    body = int(body)
    if body in layout.aliases:
        raise ValueError('link_accelerations: model %d is attached to its parent; acceleration sensing on an attached child model is not '
                         'supported' % body)
    if not 0 <= body < layout.n_bodies:
        raise ValueError('dg_world_link_accelerations: body %d out of range' % body)
    I = layout.I
    bi = I[int(I[K.H_OFF_BODY_I]) + body * K.BI_STRIDE:][:K.BI_STRIDE]
    if int(bi[K.BI_FLAGS]) & K.BODY_FROZEN:
        raise ValueError('dg_world_link_accelerations: body %d is part of the frozen static world: it never moves' % body)
    if int(bi[K.BI_PREV_OFF]) < 0:
        raise ValueError('dg_world_link_accelerations: body %d keeps no saved velocities; call builder.enable_joint_force_torque(body) while the scene '
                         'is built (imu_sensor does), or put a compiled force_torque_sensor on the body; a fixed base without joints keeps none' % body)
    frames = [-1] if frames is None else [int(f) for f in frames]
    n = len(frames)
    if not 1 <= n <= LINK_ACCEL_MAX:
        raise ValueError('link_accelerations takes 1 .. %d frames, got %d' % (LINK_ACCEL_MAX, n))
    nfr = len(layout.flats[body].frames)
    pos = np.zeros((n, 3)) if local_pos is None else np.array(local_pos, dtype=np.float64)
    orn = np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)) if local_orn is None else np.array(local_orn, dtype=np.float64)
    if pos.shape not in ((3, ), (n, 3)) or orn.shape not in ((4, ), (n, 4)):
        raise ValueError('link_accelerations: local_pos must be [3] or [%d, 3] and local_orn [4] or [%d, 4], got %s and %s' % (n, n, pos.shape, orn.shape))
    pos, orn = np.broadcast_to(pos, (n, 3)), np.broadcast_to(orn, (n, 4))
    if not (np.isfinite(pos).all() and np.isfinite(orn).all()):
        raise ValueError('link_accelerations: local_pos and local_orn must be finite')
    arr = (AccelSelector * n)()
    for k, f in enumerate(frames):
        if not -1 <= f < nfr:
            raise ValueError('dg_world_link_accelerations: body %d has no frame %d' % (body, f))
        qn = float(np.linalg.norm(orn[k]))
        if not qn > 0.0:
            raise ValueError('dg_world_link_accelerations: the mount quaternion of selector %d has zero norm' % k)
        arr[k].frame, arr[k].com = f, int(bool(com))
        arr[k].pos[:] = [float(x) for x in pos[k]]
        arr[k].quat[:] = [float(x) for x in orn[k] / qn]
    return body, arr


def joint_wrench_selectors(layout, body, joints=None):
    """The selectors ``dg_world_joint_wrench`` takes for joints ``joints`` of ``body`` (a Model's ``uid``; what
    ``Model.get_frame_id`` returns, fixed or movable; None: every movable joint), from the scene alone: ``(body index, joints,
    (JointSelector * n))``.  The child side of each joint is the compiled sensor's (``FlatBody.ft_cluster``): the rigid cluster of
    URDF links behind the joint -- the whole moving link when the joint is movable -- plus every moving link hanging off it.
    ValueError for what the entry would refuse."""
    K = _scene_constants()
    body = int(body)
    if body in layout.aliases:
        raise ValueError('joint_reaction_forces: model %d is attached to its parent; joint force/torque sensing across the joints of an attached child '
                         'model is not supported' % body)
    if not 0 <= body < layout.n_bodies:
        raise ValueError('dg_world_joint_wrench: body %d out of range' % body)
    I = layout.I
    bi = I[int(I[K.H_OFF_BODY_I]) + body * K.BI_STRIDE:][:K.BI_STRIDE]
    if int(bi[K.BI_FLAGS]) & K.BODY_FROZEN:
        raise ValueError('dg_world_joint_wrench: body %d is part of the frozen static world: it has no joints' % body)
    if int(bi[K.BI_PREV_OFF]) < 0:
        raise ValueError('dg_world_joint_wrench: body %d keeps no saved velocities; call builder.enable_joint_force_torque(body) while the scene is '
                         'built (joint_wrench_sensor does), or put a compiled force_torque_sensor on the body' % body)
    flat = layout.flats[body]
    joints = list(flat.dof_to_joint) if joints is None else [int(j) for j in joints]
    if not 1 <= len(joints) <= JOINT_WRENCH_MAX:
        raise ValueError('joint_reaction_forces takes 1 .. %d joints, got %d' % (JOINT_WRENCH_MAX, len(joints)))
    if len(flat.links) > 64 or len(flat.frames) > 64:
        raise ValueError('dg_world_joint_wrench: body %d has %d links and %d frames; the selectors\' masks cover 64' % (body, len(flat.links), len(flat.frames)))
    arr = (JointSelector * len(joints))()
    for k, j in enumerate(joints):
        if not 0 <= j < len(flat.frames):
            raise ValueError('dg_world_joint_wrench: body %d has no frame %d' % (body, j))
        try:
            cl = flat.ft_cluster(j)
        except NotImplementedError as e:   # (a body that carries a merged child model)
            raise ValueError('dg_world_joint_wrench: %s' % (e, ))
        m, c, Ic = cl['rigid']
        arr[k].frame, arr[k].flags = j, (K.FT_WHOLE_LINK if flat.robot.joints[j].movable else 0)
        arr[k].link_mask = sum(1 << d for d in cl['moving'])
        arr[k].frame_mask = sum(1 << u for u in cl['urdf_links'])
        arr[k].rigid[:] = [m, c[0], c[1], c[2], Ic[0, 0], Ic[0, 1], Ic[0, 2], Ic[1, 1], Ic[1, 2], Ic[2, 2]]
    return body, joints, arr


def closest_candidate_pairs(layout, body_a, link_a, body_b, link_b):
    """The shape pairs ``dg_world_closest`` tests for a filter, in its row order, from the scene blob alone: side A every shape of
    ``(body_a, link_a)`` in ascending shape index, side B under it every shape of ``(body_b, link_b)`` -- with ``CONTACT_ANY`` of
    any other body.  Never a pair: two shapes of one body, visual-only shapes, two shapes neither of which can move, box against
    box.  Arguments as the C entry takes them (body indices, pybullet link indices, ``CONTACT_ANY``)."""
    K = _scene_constants()
    I = layout.I
    n = int(I[K.H_N_SHAPES])
    SI = I[I[K.H_OFF_SHAPE_I]:I[K.H_OFF_SHAPE_I] + n * K.SI_STRIDE].reshape(n, K.SI_STRIDE)
    BI = I[I[K.H_OFF_BODY_I]:I[K.H_OFF_BODY_I] + layout.n_bodies * K.BI_STRIDE].reshape(layout.n_bodies, K.BI_STRIDE)
    body, link = SI[:, K.SI_BODY], ((SI[:, K.SI_FLAGS] >> 8) & 0xFFFF) - 1
    solid = (SI[:, K.SI_FLAGS] & K.SHAPE_NO_COLLIDE) == 0
    moves = ~(((BI[body, K.BI_FLAGS] & K.BODY_FIXED) != 0) & (BI[body, K.BI_N_LINKS] == 0))
    box = SI[:, K.SI_TYPE] == 1   # DG_SHAPE_BOX

    def match(b, l):
        return solid & ((b == CONTACT_ANY) | ((body == b) & ((l == CONTACT_ANY) | (link == l))))
    ma, mb = match(body_a, link_a), match(body_b, link_b)
    return [(a, c) for a in np.nonzero(ma)[0] for c in np.nonzero(mb)[0]
            if body[a] != body[c] and (moves[a] or moves[c]) and not (box[a] and box[c])]


def debug_plan(layout, num_envs, cu_count=256):
    """What ``dg_world_create`` would decide for ``num_envs`` copies of ``layout``'s scene on a GPU of ``cu_count`` compute
    units under the environment's ``DG_*`` switches, without a device: a dict keyed by the ``DG_PLAN_*`` names of
    ``include/diygym_hip.h`` in lower case (``lanes``, ``lds_bytes``, ``par``, ...), plus ``table`` -- the plan table as an
    int32 array (layout in the header)."""
    from .scene import _parse_header
    consts = {k[len('DG_PLAN_'):].lower(): v for k, v in _parse_header(os.path.join(_HERE, '..', 'include', 'diygym_hip.h')).items()
              if k.startswith('DG_PLAN_')}
    plan = {k: consts.pop(k) for k in ('plb_stride', 'pll_stride')}   # (constants of the table's layout, not slots)
    out = np.zeros(consts.pop('count'), dtype=np.int32)
    lib = load_library()
    I, F = layout.I, layout.F

    def call(table):
        rc = lib.dg_debug_plan(I.ctypes.data_as(_c_i32p), I.size, F.ctypes.data_as(_c_f64p), F.size, int(num_envs), int(cu_count),
                               out.ctypes.data_as(_c_i32p), table.ctypes.data_as(_c_i32p), table.size)
        if rc != 0:
            raise RuntimeError('diygym_hip error %d: %s' % (rc, lib.dg_last_error().decode()))
        return table

    call(np.zeros(0, dtype=np.int32))   # (for the table's length)
    plan['table'] = call(np.zeros(int(out[consts['table_words']]), dtype=np.int32))
    plan.update((name, int(out[k])) for name, k in consts.items())
    return plan


class HipBackend:
    """Owns one ``dg_world`` and the device tensors of one shard of envs."""
    def __init__(self, layout, num_envs, device=None, seed=0, env_index_base=0):
        if not torch.cuda.is_available():
            raise RuntimeError('diy_gym_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback')
        self.lib = load_library()
        self.layout = layout
        self.num_envs = int(num_envs)
        self.device = torch.device(device if device is not None else 'cuda:0')
        if self.device.type != 'cuda':
            raise RuntimeError('diy_gym_amd runs on ROCm devices only, got %s' % self.device)
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        # always indexed: tensors allocated on 'cuda' report 'cuda:<n>', and device('cuda') != device('cuda:0')
        self.device = torch.device('cuda', dev_index)
        self.stride = ((self.num_envs + 63) // 64) * 64
        I, F = layout.I, layout.F
        handle = _vp()
        rc = self.lib.dg_world_create(I.ctypes.data_as(_c_i32p), I.size, F.ctypes.data_as(_c_f64p), F.size, self.num_envs,
                                      self.stride, dev_index, ctypes.c_uint64(seed), ctypes.c_int64(env_index_base),
                                      ctypes.byref(handle))
        self._check(rc)
        self.handle = handle
        dims = (ctypes.c_int32 * 8)()
        self._check(self.lib.dg_world_dims(self.handle, dims))
        self.state_dim, self.act_dim, self.obs_dim, self.rew_dim, self.term_dim, self.n_links, self.lds_bytes, self.lanes = list(dims)
        B, dev = self.num_envs, self.device
        with torch.cuda.device(dev):
            self.state = torch.zeros((self.state_dim, self.stride), dtype=torch.float32, device=dev)
            self.act = torch.zeros((B, max(self.act_dim, 1)), dtype=torch.float32, device=dev)
            self.obs = torch.zeros((B, max(self.obs_dim, 1)), dtype=torch.float32, device=dev)
            self.rew = torch.zeros((B, max(self.rew_dim, 1)), dtype=torch.float32, device=dev)
            self.term = torch.zeros((B, max(self.term_dim, 1)), dtype=torch.uint8, device=dev)
            self.rew_sum = torch.zeros((B, ), dtype=torch.float32, device=dev)
            self.term_flag = torch.zeros((B, ), dtype=torch.uint8, device=dev)
        self._ray_scratch, self._ray_out = None, {}   # ray_test_batch: the pose scratch and the output buffers per `want`
        self._dyn_out = {}   # the dynamics queries' output buffers per (call kind, body)
        self._contact_out = {}   # contact_points: the output buffers per `want`
        self._contact_force_out, self._net_contact_out = {}, {}   # contact_forces / net_contact_forces: the output buffers per `want` (and n)
        self._closest_scratch, self._closest_out = None, {}   # closest_points: the scratch and the output buffers per (`want`, K)
        self._closest_k = {}   # ... and the default K per filter
        self._ik_list_cache = {}   # calculate_inverse_kinematics: the null-space lists on the device, per distinct value
        self._link_states_out = {}   # link_states: the selector arrays and the output buffer per (selectors, com)
        self._joint_wrench_out = {}   # joint_reaction_forces: the selectors and the output buffer per (body, joints)
        self._link_accel_out = {}   # link_accelerations: the output buffer (its pointer and its five views) per number of selectors
        self._link_accel_sel = {}   # ... and the selectors per distinct arguments
        self._check(self.lib.dg_world_init_state(self.handle, _ptr(self.state), self._stream()))

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError('diygym_hip error %d: %s' % (rc, self.lib.dg_last_error().decode()))

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.dg_world_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- argument checks ------------------------------------------------------
    # The kernels index raw device pointers: a CPU tensor, a strided view, a wrong width or a short mask would be an
    # out-of-bounds device access, not a Python error -- so every caller-supplied tensor is checked here.
    def _require(self, name, t, shape, dtype):
        if not isinstance(t, torch.Tensor):
            raise ValueError('%s must be a torch.Tensor, got %s' % (name, type(t).__name__))
        if t.device != self.device:
            raise ValueError('%s is on %s, this backend runs on %s' % (name, t.device, self.device))
        if t.dtype != dtype:
            raise ValueError('%s must be %s, got %s' % (name, dtype, t.dtype))
        if tuple(t.shape) != tuple(shape):
            raise ValueError('%s must have shape %s, got %s' % (name, tuple(shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError('%s must be contiguous' % name)
        return t

    def _require_numel(self, name, t, numel, dtype):
        if not isinstance(t, torch.Tensor):
            raise ValueError('%s must be a torch.Tensor, got %s' % (name, type(t).__name__))
        if t.device != self.device or t.dtype != dtype or not t.is_contiguous() or t.numel() != numel:
            raise ValueError('%s must be a contiguous %s tensor of %d elements on %s, got %s %s on %s' %
                             (name, dtype, numel, self.device, t.dtype, tuple(t.shape), t.device))
        return t

    def _env_mask(self, mask):
        """``mask`` (None, or one flag per env) as None or a contiguous uint8 tensor on this device."""
        if mask is not None:
            if not isinstance(mask, torch.Tensor):
                mask = torch.as_tensor(mask)
            if mask.numel() != self.num_envs:
                raise ValueError('reset mask must have one element per env (%d), got shape %s' % (self.num_envs, tuple(mask.shape)))
            if mask.dtype == torch.bool and mask.device == self.device and mask.is_contiguous():
                mask = mask.view(torch.uint8)
            elif mask.dtype != torch.uint8 or mask.device != self.device or not mask.is_contiguous():
                mask = (mask != 0).to(device=self.device, dtype=torch.uint8).contiguous()
        return mask

    # -- step path --------------------------------------------------------
    def reset(self, mask=None):
        """``mask``: None (all envs) or one flag per env; bool / uint8 masks on the backend's device are used as they
        are (a bool tensor is reinterpreted, not copied), anything else is converted."""
        mask = self._env_mask(mask)
        self._check(self.lib.dg_world_reset(self.handle, _ptr(self.state), _ptr(mask), _ptr(self.obs), self._stream()))

    def step(self, update_mask, actions=None):
        act = self.act if actions is None else self._require('actions', actions, (self.num_envs, max(self.act_dim, 1)), torch.float32)
        self._check(
            self.lib.dg_world_step(self.handle, _ptr(self.state), _ptr(act) if self.act_dim else None,
                                   ctypes.c_uint64(update_mask), _ptr(self.obs), _ptr(self.rew), _ptr(self.term),
                                   _ptr(self.rew_sum), _ptr(self.term_flag), self._stream()))

    def observe(self):
        self._check(
            self.lib.dg_world_observe(self.handle, _ptr(self.state), _ptr(self.obs), _ptr(self.rew), _ptr(self.term),
                                      _ptr(self.rew_sum), _ptr(self.term_flag), self._stream()))

    def frame_state(self, body, frame=-1, com=False):
        out = torch.empty((self.num_envs, 13), dtype=torch.float32, device=self.device)
        self._check(self.lib.dg_world_frame_state(self.handle, _ptr(self.state), int(body), int(frame), int(bool(com)), _ptr(out),
                                                  self._stream()))
        return out

    # -- batched p.getLinkStates / p.resetBasePositionAndOrientation / p.resetBaseVelocity ------------------------------------
    def link_states(self, body, frames=None, com=False):
        """``p.getLinkStates(uid, frames, computeLinkVelocity=1)`` -- and ``getBasePositionAndOrientation`` / ``getBaseVelocity``, frame
        -1 -- for every env at once, in ONE launch: ``[B, n, 13]``, row k the position (3), quaternion xyzw (4), world linear (3) and
        angular (3) velocity of frame ``frames[k]``; exactly the bits ``frame_state(body, frames[k], com)`` returns.  ``body`` is a
        Model's ``uid`` (an attached child model's alias uid included), or a list of uids as long as ``frames`` -- the poses of
        several models in one call; ``frames`` a list of up to 32 of what ``Model.get_frame_id`` returns (-1: the base; default
        ``[-1]``).  ``com``: the link's INERTIAL frame instead of its URDF frame, as in ``frame_state``.  The state is not written.
        Argument errors raise ValueError.

        The result is a view of a buffer kept per ``(selectors, com)`` and REUSED by the next call with the same arguments: clone
        what must last."""
        frames = [-1] if frames is None else [int(f) for f in frames]
        bodies = [int(b) for b in body] if isinstance(body, (list, tuple)) else [int(body)] * len(frames)
        if len(bodies) != len(frames):
            raise ValueError('link_states: %d bodies for %d frames (one uid, or one per frame)' % (len(bodies), len(frames)))
        key = (tuple(bodies), tuple(frames), bool(com))
        if key not in self._link_states_out:
            n = len(frames)
            if not 1 <= n <= LINK_STATES_MAX:
                raise ValueError('link_states takes 1 .. %d frames, got %d' % (LINK_STATES_MAX, n))
            sel = []
            for uid, f in zip(bodies, frames):
                if f < -1:
                    raise ValueError('link_states: frame must be a frame id (-1: the base), got %d' % f)
                b, lf = self.layout.resolve_frame(uid, f)   # (the uid of a merged child model is an alias into its parent's body)
                if not 0 <= b < self.layout.n_bodies:
                    raise ValueError('link_states: body %d is not a model of this scene' % uid)
                if lf >= self._body_n_frames(b):
                    raise ValueError('link_states: body %d has no frame %d' % (uid, f))
                sel.append((b, lf))
            self._link_states_out[key] = ((ctypes.c_int32 * n)(*[b for b, _ in sel]), (ctypes.c_int32 * n)(*[f for _, f in sel]),
                                          torch.empty((self.num_envs, n, 13), dtype=torch.float32, device=self.device))
        b_arr, f_arr, out = self._link_states_out[key]
        self._dyn_check(self.lib.dg_world_link_states(self.handle, _ptr(self.state), b_arr, f_arr, len(frames), int(bool(com)), _ptr(out), self._stream()))
        return out

    def base_is_movable(self, body):
        """Whether ``reset_base_state`` takes the body (an index, not an alias): a floating base, or a fixed base that carries a
        ``respawn`` op -- the planner pins every other fixed base to its load pose (static pair pruning, anchored bounding spheres)."""
        K = _scene_constants()
        I = self.layout.I
        if not self.layout.body_fixed[body]:
            return True
        if int(I[int(I[K.H_OFF_BODY_I]) + body * K.BI_STRIDE + K.BI_FLAGS]) & K.BODY_FROZEN:
            return False
        n, off = int(I[K.H_N_OPS]), int(I[K.H_OFF_OP_I])
        OI = I[off:off + n * K.OI_STRIDE].reshape(n, K.OI_STRIDE)
        return bool(((OI[:, K.OI_CODE] == K.OP_RESPAWN) & (OI[:, K.OI_BODY] == body)).any())

    def _rows4(self, name, v):
        """``v`` as a contiguous float32 ``[num_envs, 4]`` tensor on this device: one quaternion for every env, or one per env."""
        if v is None:
            return None
        t = torch.as_tensor(v, dtype=torch.float32, device=self.device) if not isinstance(v, torch.Tensor) else v.to(device=self.device, dtype=torch.float32)
        if t.numel() == 4:
            t = t.reshape(1, 4).expand(self.num_envs, 4)
        if t.numel() != 4 * self.num_envs:
            raise ValueError('%s must have 4 or %d x 4 elements, got shape %s' % (name, self.num_envs, tuple(t.shape)))
        return t.reshape(self.num_envs, 4).contiguous()

    def reset_base_state(self, body, pos=None, orn=None, lin_vel=None, ang_vel=None, mask=None):
        """``p.resetBasePositionAndOrientation(uid, pos, orn)`` and ``p.resetBaseVelocity(uid, lin_vel, ang_vel)`` for the envs
        ``mask`` selects (as for ``reset``; default all).  ``pos`` (``[B, 3]`` or one 3-vector) and ``orn`` (``[B, 4]`` or ``[4]``,
        xyzw; normalised on the device) go together: the pose of the base's INERTIAL frame, what ``frame_state(uid, -1, com=True)``
        reports and what the ``respawn`` addon sets.  ``lin_vel`` / ``ang_vel`` (``[B, 3]`` or one 3-vector) are the world velocity of
        that frame's origin and the world angular velocity, columns 7:13 of the same report.  With a pose, a velocity that is not
        given becomes zero, as in pybullet; without one only the given velocities change.  Joint state, motor targets and pending
        external forces stay; the reset envs' contact impulse cache is emptied.  Observations are refreshed by the next
        ``observe()`` or ``step()``.

        The body must be one whose base the scene lets move: a floating base, or a fixed base with a ``respawn`` addon (zero ranges
        will do); a fixed base takes no velocity.  Argument errors raise ValueError."""
        if int(body) in self.layout.aliases:
            raise ValueError('reset_base_state: model %d is attached to its parent and has no base of its own' % int(body))
        body = int(body)
        if not 0 <= body < self.layout.n_bodies:
            raise ValueError('dg_world_reset_base_state: body %d out of range' % body)
        if (pos is None) != (orn is None):
            raise ValueError('dg_world_reset_base_state: pos and orn go together (both or neither)')
        if pos is None and lin_vel is None and ang_vel is None:
            raise ValueError('dg_world_reset_base_state: nothing to write (pos, orn, lin_vel and ang_vel are all NULL)')
        if not self.base_is_movable(body):
            raise ValueError('dg_world_reset_base_state: body %d has a fixed base that the scene pins to its load pose; add a respawn addon to the model '
                             '(zero ranges will do) to make its base movable' % body)
        if self.layout.body_fixed[body] and (lin_vel is not None or ang_vel is not None):
            raise ValueError('dg_world_reset_base_state: body %d has a fixed base: it takes a pose, no velocity' % body)
        pos, orn = self._rows3('pos', pos), self._rows4('orn', orn)
        lin_vel, ang_vel = self._rows3('lin_vel', lin_vel), self._rows3('ang_vel', ang_vel)
        self._dyn_check(self.lib.dg_world_reset_base_state(self.handle, _ptr(self.state), body, _ptr(pos), _ptr(orn), _ptr(lin_vel), _ptr(ang_vel),
                                                           _ptr(self._env_mask(mask)), self._stream()))

    # -- batched p.applyExternalForce / p.applyExternalTorque for addons written in Python ----------------------------
    LINK_FRAME, WORLD_FRAME = 1, 2   # pybullet's flag values

    def _rows3(self, name, v):
        """``v`` as a contiguous float32 ``[num_envs, 3]`` tensor on this device: one 3-vector for every env, or one per env."""
        if v is None:
            return None
        t = torch.as_tensor(v, dtype=torch.float32, device=self.device) if not isinstance(v, torch.Tensor) else v.to(device=self.device, dtype=torch.float32)
        if t.numel() == 3:
            t = t.reshape(1, 3).expand(self.num_envs, 3)
        if t.numel() != 3 * self.num_envs:
            raise ValueError('%s must have 3 or %d x 3 elements, got shape %s' % (name, self.num_envs, tuple(t.shape)))
        return t.reshape(self.num_envs, 3).contiguous()

    def apply_external_force(self, body, frame, force, pos=None, flags=2):
        """``p.applyExternalForce(uid, linkIndex, forceObj, posObj, flags)`` for every env at once (``force``: ``[B, 3]`` or
        one 3-vector; ``pos``: likewise, default the origin).  ``body`` is a Model's ``uid`` (an attached child model's alias
        uid included), ``frame`` the index ``Model.get_frame_id`` returns (-1: the base).  ``LINK_FRAME`` means the link's
        INERTIAL frame, as in pybullet.  The force acts during the next ``step`` only; see ``dg_world_apply_wrench``."""
        body, frame = self.layout.resolve_frame(body, frame)   # (the uid of a merged child model is an alias into its parent's body)
        # (the converted rows are held until the launch is queued: a temporary dropped right after _ptr() hands its block back to
        # the allocator, and the next conversion gets the same block -- force and pos would then read the same memory)
        f, p = self._rows3('force', force), self._rows3('pos', pos)
        self._check(self.lib.dg_world_apply_wrench(self.handle, _ptr(self.state), int(body), int(frame), int(flags), _ptr(f), _ptr(p), None, self._stream()))

    def apply_external_wrench(self, body, frame, force, pos, torque, flags=2):
        """Force at ``pos`` and torque in ONE launch (what the compiled ``propellor`` op does: its base torque is
        ``r x F + T`` summed before it is added to the state, so this form reproduces that op bit for bit)."""
        body, frame = self.layout.resolve_frame(body, frame)
        f, p, t = self._rows3('force', force), self._rows3('pos', pos), self._rows3('torque', torque)   # (held until the launch is queued)
        self._check(self.lib.dg_world_apply_wrench(self.handle, _ptr(self.state), int(body), int(frame), int(flags), _ptr(f), _ptr(p), _ptr(t), self._stream()))

    def apply_external_torque(self, body, frame, torque, flags=2):
        """``p.applyExternalTorque(uid, linkIndex, torqueObj, flags)`` for every env at once."""
        body, frame = self.layout.resolve_frame(body, frame)
        t = self._rows3('torque', torque)
        self._check(self.lib.dg_world_apply_wrench(self.handle, _ptr(self.state), int(body), int(frame), int(flags), None, None, _ptr(t), self._stream()))

    def camera_resolution(self, camera):
        I, K = self.layout.I, _scene_constants()
        if not 0 <= int(camera) < int(I[K.H_N_CAMERAS]):
            raise ValueError('camera %d out of range (scene has %d)' % (camera, int(I[K.H_N_CAMERAS])))
        ci = I[I[K.H_OFF_CAMERA_I] + int(camera) * K.CI_STRIDE:]
        return int(ci[K.CI_WIDTH]), int(ci[K.CI_HEIGHT])

    def render(self, camera, rgb=None, depth=None, seg=None):
        w, h = self.camera_resolution(camera)
        px = self.num_envs * w * h
        if rgb is not None:
            self._require_numel('rgb', rgb, 3 * px, torch.float32)
        if depth is not None:
            self._require_numel('depth', depth, px, torch.float32)
        if seg is not None:
            self._require_numel('seg', seg, px, torch.int32)
        self._check(self.lib.dg_world_render(self.handle, _ptr(self.state), int(camera), _ptr(rgb), _ptr(depth), _ptr(seg), self._stream()))

    # -- batched p.rayTestBatch ------------------------------------------------------------------------------------------
    def ray_test_batch(self, ray_from, ray_to, body=-1, frame=-1, skip_body=-1, want=('frac', 'id', 'pos', 'normal')):
        """``p.rayTestBatch(rayFromPositions, rayToPositions)`` for every env at once: ``ray_from`` / ``ray_to`` are float32
        ``[N, 3]`` (the same rays in every env) or ``[B, N, 3]`` (rays of their own per env) on this device -- in world
        coordinates, or with ``body`` (a Model's ``uid``) in the frame ``frame`` of that model (the index
        ``Model.get_frame_id`` returns, -1: the base), which is what a sensor riding on a link wants.  ``skip_body``: a
        model no ray can hit (the sensor's own).  Returns ``RayHits(frac, id, pos, normal)``: ``[B, N]`` hit fraction (1.0 =
        nothing hit), ``[B, N]`` int32 ``uid + ((link + 1) << 24)`` (-1 = nothing hit), ``[B, N, 3]`` world hit position
        (``ray_to`` on a miss) and ``[B, N, 3]`` world unit normal (0 on a miss); those not named in ``want`` are None.  The
        tensors are views of buffers kept per ``want`` (grown to the largest N seen) and REUSED by the next call: clone what must last.
        See ``dg_world_raycast`` for the semantics."""
        B = self.num_envs
        if not isinstance(ray_from, torch.Tensor) or not isinstance(ray_to, torch.Tensor):
            raise ValueError('ray_from and ray_to must be torch.Tensors')
        if ray_from.dim() not in (2, 3) or ray_from.shape[-1] != 3 or ray_from.shape[-2] < 1:
            raise ValueError('ray_from must have shape [N, 3] or [%d, N, 3] with N >= 1, got %s' % (B, tuple(ray_from.shape)))
        per_env, n = ray_from.dim() == 3, int(ray_from.shape[-2])
        shape = (B, n, 3) if per_env else (n, 3)
        self._require('ray_from', ray_from, shape, torch.float32)
        self._require('ray_to', ray_to, shape, torch.float32)
        unknown = set(want) - set(RayHits._fields)
        if unknown or 'frac' not in want:
            raise ValueError("want must name 'frac' and any of 'id', 'pos', 'normal', got %r" % (want, ))
        if body >= 0:
            body, frame = self.layout.resolve_frame(body, frame)
        if skip_body >= 0:
            skip_body = self.layout.resolve_frame(skip_body, -1)[0]
        # one set of flat output buffers per `want`, grown to the largest N seen; the [B, N] results are views of their heads
        key = tuple(f in want for f in RayHits._fields)
        if self._ray_scratch is None:
            self._ray_scratch = torch.empty((max(int(self.lib.dg_world_raycast_scratch_floats(self.handle)), 1), ), dtype=torch.float32, device=self.device)
        if key not in self._ray_out or self._ray_out[key][0].numel() < B * n:
            self._ray_out[key] = (torch.empty((B * n, ), dtype=torch.float32, device=self.device),
                                  torch.empty((B * n, ), dtype=torch.int32, device=self.device) if key[1] else None,
                                  torch.empty((B * n * 3, ), dtype=torch.float32, device=self.device) if key[2] else None,
                                  torch.empty((B * n * 3, ), dtype=torch.float32, device=self.device) if key[3] else None)
        f_, i_, p_, n_ = self._ray_out[key]
        out = RayHits(f_[:B * n].view(B, n), None if i_ is None else i_[:B * n].view(B, n), None if p_ is None else p_[:3 * B * n].view(B, n, 3),
                      None if n_ is None else n_[:3 * B * n].view(B, n, 3))
        self._check(self.lib.dg_world_raycast(self.handle, _ptr(self.state), int(body), int(frame), n, _ptr(ray_from), _ptr(ray_to), int(per_env),
                                              int(skip_body), _ptr(self._ray_scratch), _ptr(out.frac), _ptr(out.id), _ptr(out.pos), _ptr(out.normal),
                                              self._stream()))
        return out

    # -- batched p.getJointStates / p.calculateJacobian / p.calculateInverseDynamics / p.calculateMassMatrix / TORQUE_CONTROL ----
    # For addons written in Python (an operational-space or computed-torque controller ported from pybullet; reference
    # diy_gym/addons/controllers/admittance_controller.py:36-55).  Fixed-base bodies with at least one joint only: anything else
    # raises ValueError.  ``body`` is a Model's ``uid``; the uid of a child model merged into its parent is an alias of the
    # PARENT's body, so ``nv`` -- the number of joints, the width of every vector below -- is then the parent's, in the order of
    # the merged body's joints.  Vectors are float32 ``[B, nv]`` on this device (or one ``[nv]`` vector for every env).  Outputs
    # are buffers kept per call kind and body and REUSED by the next call of that kind: clone what must last.
    def _dyn_check(self, rc):
        if rc == -4:   # DG_ERR_ARG: a body or frame the queries do not take
            raise ValueError(self.lib.dg_last_error().decode())
        self._check(rc)

    def _dyn_body(self, body, frame=-1):
        """``(body index, body-local frame, nv)``; ValueError for a body the dynamics queries do not take."""
        body, frame = self.layout.resolve_frame(body, frame)
        if not 0 <= body < self.layout.n_bodies:
            raise ValueError('body %d out of range' % body)
        nv = int(self.layout.body_n_links[body])
        if not self.layout.body_fixed[body] or nv < 1:
            raise ValueError('body %d is not a fixed-base body with joints: the dynamics queries take no other' % body)
        return body, frame, nv

    def _rows_nv(self, name, v, nv):
        """``v`` (float32, this device) as a contiguous ``[num_envs, nv]`` tensor: one ``[nv]`` vector for every env, or one per env."""
        if v is None:
            return None
        if isinstance(v, torch.Tensor) and v.dim() == 1:   # broadcast into a buffer kept per argument: no allocation per call
            buf = self._dyn_buf('in_' + name, nv, self.num_envs, nv)
            buf.copy_(self._require(name, v, (nv, ), torch.float32).reshape(1, nv))
            return buf
        return self._require(name, v, (self.num_envs, nv), torch.float32)

    def _dyn_buf(self, kind, body, *shape):
        key = (kind, body)
        if key not in self._dyn_out:
            self._dyn_out[key] = torch.zeros(shape, dtype=torch.float32, device=self.device)
        return self._dyn_out[key]

    def joint_states(self, body):
        """``p.getJointStates`` (positions and velocities) for every env: ``(q, qd)``, each ``[B, nv]``."""
        body, _, nv = self._dyn_body(body)
        q, qd = self._dyn_buf('q', body, self.num_envs, nv), self._dyn_buf('qd', body, self.num_envs, nv)
        self._dyn_check(self.lib.dg_world_joint_state(self.handle, _ptr(self.state), body, _ptr(q), _ptr(qd), self._stream()))
        return q, qd

    def calculate_jacobian(self, body, frame, local_pos=(0.0, 0.0, 0.0), q=None):
        """``p.calculateJacobian(uid, linkIndex, localPosition, q, ...)`` for every env: ``(jac_t, jac_r)``, each ``[B, 3, nv]`` in
        world coordinates.  ``frame`` is the index ``Model.get_frame_id`` returns (>= 0), ``local_pos`` three numbers in the
        link's INERTIAL frame, ``q`` the joint positions to evaluate at (default: each env's current ones).  When ``body`` is a
        merged child's alias the frame lands on the parent's body and ``nv`` is the parent's."""
        if int(frame) < 0:
            raise ValueError('frame must be a frame id >= 0, got %d' % int(frame))
        body, frame, nv = self._dyn_body(body, frame)
        lp = np.asarray(local_pos, dtype=np.float32).reshape(-1)
        if lp.size != 3:
            raise ValueError('local_pos must have 3 elements, got %d' % lp.size)
        q = self._rows_nv('q', q, nv)
        jt, jr = self._dyn_buf('jac_t', body, self.num_envs, 3, nv), self._dyn_buf('jac_r', body, self.num_envs, 3, nv)
        self._dyn_check(self.lib.dg_world_jacobian(self.handle, _ptr(self.state), body, frame, (ctypes.c_float * 3)(*lp.tolist()), _ptr(q), _ptr(jt), _ptr(jr),
                                                   self._stream()))
        return jt, jr

    def calculate_inverse_dynamics(self, body, q=None, qd=None, qdd=None):
        """``p.calculateInverseDynamics(uid, q, qd, qdd)`` for every env: ``[B, nv]`` joint torques ``M qdd + C qd - G`` (rigid-body
        terms only).  ``q`` / ``qd`` default to each env's current values, ``qdd`` to zero; with ``qd`` and ``qdd`` zero the
        result is the gravity compensation."""
        body, _, nv = self._dyn_body(body)
        q, qd, qdd = self._rows_nv('q', q, nv), self._rows_nv('qd', qd, nv), self._rows_nv('qdd', qdd, nv)
        tau = self._dyn_buf('tau', body, self.num_envs, nv)
        self._dyn_check(self.lib.dg_world_inverse_dynamics(self.handle, _ptr(self.state), body, _ptr(q), _ptr(qd), _ptr(qdd), _ptr(tau), self._stream()))
        return tau

    def calculate_mass_matrix(self, body, q=None):
        """``p.calculateMassMatrix(uid, q)`` for every env: ``[B, nv, nv]``, symmetric bit for bit."""
        body, _, nv = self._dyn_body(body)
        q = self._rows_nv('q', q, nv)
        M = self._dyn_buf('M', body, self.num_envs, nv, nv)
        self._dyn_check(self.lib.dg_world_mass_matrix(self.handle, _ptr(self.state), body, _ptr(q), _ptr(M), self._stream()))
        return M

    def apply_joint_torque(self, body, torque):
        """``p.setJointMotorControlArray(uid, joints, p.TORQUE_CONTROL, forces=torque)`` for every env: ``torque`` (``[B, nv]`` or
        ``[nv]``) is ADDED to the joints' torques for the next ``step`` only, on top of what compiled addons apply."""
        body, _, nv = self._dyn_body(body)
        if torque is None:
            raise ValueError('torque must be a torch.Tensor, got None')
        self._dyn_check(self.lib.dg_world_apply_joint_torque(self.handle, _ptr(self.state), body, _ptr(self._rows_nv('torque', torque, nv)), self._stream()))

    # -- task-space dynamics: what an operational-space controller needs per tick, in one launch ------------------------------
    def task_space_dynamics(self, body, frame, local_pos=(0.0, 0.0, 0.0), axes=(0, 1, 2, 3, 4, 5), q=None, qd=None, acc=None, tau_null=None, damping=0.0,
                            want=('jac', 'bias_acc', 'bias_torque', 'lambda', 'tau', 'point', 'singular')):
        """The task-space dynamics of the point ``local_pos`` (INERTIAL frame of ``frame``'s link, as ``calculate_jacobian`` takes
        it) for every env in ONE launch (``dg_world_task_space``).  The task vector is ``[v; w]`` of the point in world axes;
        ``axes`` names the ``m`` rows kept (distinct indices 0 .. 5, taken in increasing order).  ``q`` / ``qd`` default to each
        env's current values; ``acc`` ``[B, m]`` is the desired task acceleration, ``tau_null`` ``[B, nv]`` a joint torque applied
        through the dynamically consistent null-space projector, ``damping`` >= 0 is added to the diagonal of ``J M^-1 J^T``.
        Returns a ``TaskSpaceDynamics``: ``jac [B, m, nv]``, ``bias_acc [B, m]`` (``Jdot qd``), ``bias_torque [B, nv]``
        (``C qd - G``), ``lambda_ [B, m, m]`` (``(J M^-1 J^T + damping I)^-1``, symmetric in bits; ``want`` spells it ``'lambda'``),
        ``tau [B, nv]`` (``J^T Lambda (acc - Jdot qd) + h + N^T tau_null``), ``point [B, 13]`` (position, quaternion xyzw of the
        link's inertial frame, linear and angular velocity) and ``singular [B]`` int32 (1: a pivot sat at the floor, see the C
        header).  Fields not in ``want`` are None; ``tau`` leaves the default ``want`` when ``acc`` is None.  The tensors are
        views of buffers kept per ``(m, want)`` and REUSED by the next call: clone what must last.  ValueError, before anything is
        launched, for everything the entry refuses (a body or frame the dynamics queries do not take, no or bad ``axes``, more rows
        than joints, a negative or non-finite ``damping``, an empty ``want``, ``'tau'`` without ``acc``, ``tau_null`` without
        ``'tau'``) and for tensors of the wrong shape, dtype or device."""
        if int(frame) < 0:
            raise ValueError('frame must be a frame id >= 0, got %d' % int(frame))
        body, frame, nv = self._dyn_body(body, frame)
        lp = np.asarray(local_pos, dtype=np.float32).reshape(-1)
        if lp.size != 3:
            raise ValueError('local_pos must have 3 elements, got %d' % lp.size)
        axes = [int(a) for a in axes]
        if len(set(axes)) != len(axes) or any(a < 0 for a in axes):
            raise ValueError('axes must be distinct indices 0 .. 5 of [v; w], got %r' % (axes, ))
        # what the shapes below depend on is refused here, in the entry's words; the entry refuses the rest before it launches
        m, mask = len(axes), sum(1 << min(a, 30) for a in axes)
        if mask <= 0 or mask > 63:
            raise ValueError('dg_world_task_space: axes_mask %d selects no row or a row above 5 of [v; w]' % mask)
        if m > nv:
            raise ValueError('dg_world_task_space: %d task rows for a body of %d joints' % (m, nv))
        fields = TaskSpaceDynamics._fields
        every = tuple(f.rstrip('_') for f in fields)
        names = ['lambda_' if n == 'lambda' else n for n in want]
        if set(names) - set(fields):
            raise ValueError('want must name some of %r, got %r' % (every, want))
        if acc is None and tuple(want) == every:   # (the default)
            names.remove('tau')
        q, qd, tau_null = self._rows_nv('q', q, nv), self._rows_nv('qd', qd, nv), self._rows_nv('tau_null', tau_null, nv)
        acc = self._rows_nv('acc', acc, m)
        key = ('task_space', body, m, tuple(f in names for f in fields))
        if key not in self._dyn_out:
            B = self.num_envs
            shapes = {'jac': (B, m, nv), 'bias_acc': (B, m), 'bias_torque': (B, nv), 'lambda_': (B, m, m), 'tau': (B, nv), 'point': (B, 13), 'singular': (B, )}
            self._dyn_out[key] = TaskSpaceDynamics(*[torch.zeros(shapes[f], dtype=torch.int32 if f == 'singular' else torch.float32, device=self.device)
                                                     if f in names else None for f in fields])
        out = self._dyn_out[key]
        self._dyn_check(self.lib.dg_world_task_space(self.handle, _ptr(self.state), body, frame, (ctypes.c_float * 3)(*lp.tolist()), mask, _ptr(q), _ptr(qd),
                                                     _ptr(acc), _ptr(tau_null), float(damping), *[_ptr(t) for t in out], self._stream()))
        return out

    # -- forward dynamics and K-sample joint-space rollouts through the body's own model ---------------------------------------
    def calculate_forward_dynamics(self, body, q=None, qd=None, tau=None, joint_damping=False, return_singular=False):
        """``qdd = M(q)^-1 (tau - h(q, qd))`` for every env in ONE launch (``dg_world_forward_dynamics``): ``[B, nv]``, the inverse
        of ``calculate_inverse_dynamics`` (rigid-body terms only).  ``q`` / ``qd`` default to each env's current values, ``tau``
        to zero; with ``joint_damping`` the joints' URDF damping x ``qd`` comes off ``tau`` first, as in the step.  With
        ``return_singular`` the result is ``(qdd, singular)``, ``singular`` ``[B]`` int32 (1: a pivot of M's factorisation sat at
        the floor, see the C header).  Buffers kept per body and REUSED by the next call: clone what must last."""
        body, _, nv = self._dyn_body(body)
        q, qd, tau = self._rows_nv('q', q, nv), self._rows_nv('qd', qd, nv), self._rows_nv('tau', tau, nv)
        qdd = self._dyn_buf('qdd', body, self.num_envs, nv)
        sing = None
        if return_singular:
            key = ('fd_singular', body)
            if key not in self._dyn_out:
                self._dyn_out[key] = torch.zeros((self.num_envs, ), dtype=torch.int32, device=self.device)
            sing = self._dyn_out[key]
        self._dyn_check(self.lib.dg_world_forward_dynamics(self.handle, _ptr(self.state), body, _ptr(q), _ptr(qd), _ptr(tau), int(bool(joint_damping)), _ptr(qdd),
                                                           _ptr(sing), self._stream()))
        return (qdd, sing) if return_singular else qdd

    def rollout_joint_dynamics(self, body, tau, q0=None, qd0=None, dt=None, frame=None, local_pos=(0.0, 0.0, 0.0), joint_damping=False, want=('q', 'qd')):
        """``K`` candidate torque sequences per env rolled ``T`` steps through the body's rigid-body model in ONE launch
        (``dg_world_rollout``): the inner loop of sampling MPC and shooting methods.  ``tau`` is ``[B, K, T, nv]`` float32 on this
        device; sample ``k`` of env ``e`` starts at ``q0[e]``, ``qd0[e]`` (``[B, nv]`` or ``[nv]``; default: the env's current
        values) and takes ``qdd = calculate_forward_dynamics(q, qd, tau[e, k, t])``, ``qd += dt qdd``, ``q += dt qd`` -- the step's
        order; ``dt`` defaults to the scene's substep.  Returns a ``JointRollout``: ``q``, ``qd`` ``[B, K, T, nv]``, ``pos``
        ``[B, K, T, 3]`` -- the world position of the point ``local_pos`` of the inertial frame of ``frame``'s link, as
        ``calculate_jacobian`` takes it; ``'pos'`` in ``want`` needs ``frame`` -- and ``singular`` ``[B, K]`` int32; row ``t`` is
        the state AFTER step ``t + 1``.  Fields not in ``want`` are None and cost nothing.  The env's per-env masses apply; the
        state is not written.  A MODEL, not the step: no joint limits, motors, link damping or contacts.  The tensors are views
        of buffers kept per ``(want, K, T)`` and REUSED by the next call: clone what must last.  ValueError, before anything is
        launched, for everything the entry refuses and for tensors of the wrong shape, dtype or device."""
        fields = JointRollout._fields
        names = list(want)
        if set(names) - set(fields):
            raise ValueError('want must name some of %r, got %r' % (fields, want))
        if 'pos' in names and frame is None:
            raise ValueError("rollout_joint_dynamics: 'pos' in want needs frame")
        if frame is not None and int(frame) < 0:
            raise ValueError('frame must be a frame id >= 0, got %d' % int(frame))
        body, frame, nv = self._dyn_body(body, -1 if frame is None else frame)
        lp = np.asarray(local_pos, dtype=np.float32).reshape(-1)
        if lp.size != 3:
            raise ValueError('local_pos must have 3 elements, got %d' % lp.size)
        if tau is None:
            raise ValueError('dg_world_rollout: tau is NULL')
        if not isinstance(tau, torch.Tensor) or tau.dim() != 4:
            raise ValueError('tau must be a torch.Tensor of shape [B, K, T, nv]')
        K, T = int(tau.shape[1]), int(tau.shape[2])
        tau = self._require('tau', tau, (self.num_envs, K, T, nv), torch.float32)
        q0, qd0 = self._rows_nv('q0', q0, nv), self._rows_nv('qd0', qd0, nv)
        dt = float(self.layout.dt if dt is None else dt)
        key = ('rollout', body, K, T, tuple(f in names for f in fields))
        if key not in self._dyn_out:
            B = self.num_envs
            shapes = {'q': (B, K, T, nv), 'qd': (B, K, T, nv), 'pos': (B, K, T, 3), 'singular': (B, K)}
            self._dyn_out[key] = JointRollout(*[torch.zeros(shapes[f], dtype=torch.int32 if f == 'singular' else torch.float32, device=self.device)
                                                if f in names else None for f in fields])
        out = self._dyn_out[key]
        self._dyn_check(self.lib.dg_world_rollout(self.handle, _ptr(self.state), body, frame, (ctypes.c_float * 3)(*lp.tolist()), K, T, dt, int(bool(joint_damping)),
                                                  _ptr(q0), _ptr(qd0), _ptr(tau), *[_ptr(t) for t in out], self._stream()))
        return out

    def rollout_joint_feedback(self, body, tau, gain=None, q_ref=None, qd_ref=None, dtau=None, alphas=None, q0=None, qd0=None, dt=None, frame=None,
                               local_pos=(0.0, 0.0, 0.0), joint_damping=False, tau_limit=None, want=('q', 'qd', 'tau')):
        """``rollout_joint_dynamics`` with the torque of every step formed INSIDE the loop, in ONE launch (``dg_world_rollout_feedback``):
        the forward pass and line search of iLQR / DDP, and the model evaluation of any time-varying feedback policy.  Sample ``k`` of
        env ``e`` takes, at the state ``q_t, qd_t`` BEFORE step ``t``, ``tau = tau[e, t] + alphas[k] dtau[e, t] + gain[e, t] @
        [q_t - q_ref[e, t]; qd_t - qd_ref[e, t]]``, clamped joint by joint to ``+-tau_limit`` where that is ``> 0``.  ``tau``,
        ``dtau``, ``q_ref``, ``qd_ref`` are ``[B, T, nv]``, ``gain`` ``[B, T, nv, 2 nv]`` (columns ``[q | qd]``; needs both
        references), ``alphas`` a sequence or ``[K]`` tensor (``K = len(alphas)``, 1 without), ``tau_limit`` ``[nv]``.  A term that is
        None is absent: with ``tau`` alone the result is ``rollout_joint_dynamics``' of ``tau`` repeated over ``K``, bit for bit.
        Returns a ``FeedbackRollout``: ``q``, ``qd``, ``tau`` ``[B, K, T, nv]`` (``tau``: the torque applied in step ``t``, after
        clamping), ``pos`` ``[B, K, T, 3]`` and ``singular`` ``[B, K]``; rows, ``q0``, ``qd0``, ``dt``, ``frame``, ``local_pos``,
        ``joint_damping`` and ``want`` as ``rollout_joint_dynamics``'.  The tensors are views of buffers kept per ``(want, K, T)``
        and REUSED by the next call: clone what must last.  ValueError, before anything is launched, for everything the entry
        refuses and for tensors of the wrong shape, dtype or device."""
        fields = FeedbackRollout._fields
        names = list(want)
        if set(names) - set(fields):
            raise ValueError('want must name some of %r, got %r' % (fields, want))
        if 'pos' in names and frame is None:
            raise ValueError("rollout_joint_feedback: 'pos' in want needs frame")
        if frame is not None and int(frame) < 0:
            raise ValueError('frame must be a frame id >= 0, got %d' % int(frame))
        body, frame, nv = self._dyn_body(body, -1 if frame is None else frame)
        lp = np.asarray(local_pos, dtype=np.float32).reshape(-1)
        if lp.size != 3:
            raise ValueError('local_pos must have 3 elements, got %d' % lp.size)
        if tau is None:
            raise ValueError('dg_world_rollout_feedback: tau_ff is NULL')
        if not isinstance(tau, torch.Tensor) or tau.dim() != 3:
            raise ValueError('tau must be a torch.Tensor of shape [B, T, nv]')
        B, T = self.num_envs, int(tau.shape[1])
        tau = self._require('tau', tau, (B, T, nv), torch.float32)
        rows = [None if v is None else self._require(name, v, (B, T, nv), torch.float32) for name, v in (('dtau', dtau), ('q_ref', q_ref), ('qd_ref', qd_ref))]
        gain = None if gain is None else self._require('gain', gain, (B, T, nv, 2 * nv), torch.float32)
        if alphas is not None and not isinstance(alphas, torch.Tensor):
            alphas = torch.tensor([float(a) for a in alphas], dtype=torch.float32, device=self.device)
        K = 1 if alphas is None else int(alphas.numel())
        if alphas is not None:
            alphas = self._require('alphas', alphas, (K, ), torch.float32)
        if tau_limit is not None and not isinstance(tau_limit, torch.Tensor):
            tau_limit = torch.tensor([float(a) for a in tau_limit], dtype=torch.float32, device=self.device)
        if tau_limit is not None:
            tau_limit = self._require('tau_limit', tau_limit, (nv, ), torch.float32)
        q0, qd0 = self._rows_nv('q0', q0, nv), self._rows_nv('qd0', qd0, nv)
        dt = float(self.layout.dt if dt is None else dt)
        key = ('rollout_feedback', body, K, T, tuple(f in names for f in fields))
        fresh = key not in self._dyn_out
        if fresh:
            shapes = {'q': (B, K, T, nv), 'qd': (B, K, T, nv), 'tau': (B, K, T, nv), 'pos': (B, K, T, 3), 'singular': (B, K)}
            self._dyn_out[key] = FeedbackRollout(*[torch.zeros(shapes[f], dtype=torch.int32 if f == 'singular' else torch.float32, device=self.device)
                                                   if f in names else None for f in fields])
        out = self._dyn_out[key]
        try:
            self._dyn_check(self.lib.dg_world_rollout_feedback(self.handle, _ptr(self.state), body, frame, (ctypes.c_float * 3)(*lp.tolist()), K, T, dt,
                                                               int(bool(joint_damping)), _ptr(q0), _ptr(qd0), _ptr(tau), _ptr(rows[0]), _ptr(alphas), _ptr(gain),
                                                               _ptr(rows[1]), _ptr(rows[2]), _ptr(tau_limit), *[_ptr(t) for t in out], self._stream()))
        except ValueError:
            if fresh:   # a refused call keeps no buffers
                del self._dyn_out[key]
            raise
        return out

    def _lq_rows(self, name, v, tail):
        """``v`` for ``lq_backward_pass``: a float32 tensor on this device whose trailing dimensions are ``tail``, as ``[B, P, *tail]``
        (a view; ``tail`` alone is one for every env and step, ``[B, *tail]`` one per env)."""
        if not isinstance(v, torch.Tensor):
            raise ValueError('%s must be a torch.Tensor, got %s' % (name, type(v).__name__))
        if v.device != self.device or v.dtype != torch.float32:
            raise ValueError('%s must be a torch.float32 tensor on %s, got %s on %s' % (name, self.device, v.dtype, v.device))
        k, B = len(tail), self.num_envs
        if tuple(v.shape[v.dim() - k:]) != tuple(tail) or v.dim() - k > 2 or (v.dim() - k >= 1 and v.shape[0] != B):
            raise ValueError('%s must have shape %s, [B = %d] + that or [B, P] + that, got %s' % (name, tuple(tail), B, tuple(v.shape)))
        if v.dim() == k:
            return v.expand((B, 1) + tuple(tail))
        return v.unsqueeze(1) if v.dim() == k + 1 else v

    def lq_backward_pass(self, body, A_q, A_v, Minv, dt, lxx, luu, lxx_T, lx=None, lu=None, lx_T=None, mu=None, horizon=None, substeps=1, want=('K', 'k', 'dV')):
        """The Riccati / iLQR backward pass of the body's joint-space model for every env in ONE launch (``dg_world_lq_backward``),
        computed in float64 from float32 tensors.  ``A_q``, ``A_v``, ``Minv`` are the CONTINUOUS derivatives exactly as
        ``forward_dynamics_derivatives(..., want=('dqdd_dq', 'dqdd_dqd', 'dqdd_dtau'))`` returns them: ``[B, T, nv, nv]`` along a
        trajectory, or ``[B, nv, nv]`` / ``[B, 1, nv, nv]`` for the stationary case, where ``horizon`` gives ``T``.  The kernel forms
        ``A, B`` itself over ``substeps`` substeps of ``dt`` (``lqr_discretise``'s formulas).  Running cost ``lxx`` (``m x m``,
        ``m = 2 nv``, state ``[dq; qd]``), ``luu`` (``nv x nv``), gradients ``lx``, ``lu`` (None = zero), terminal ``lxx_T``, ``lx_T``;
        each as one matrix / vector for every env and step, one per env (``[B, ..]``) or one per env and step (``[B, T, ..]``; not the
        terminal ones).  ``mu`` (a number or ``[B]``) is added to the diagonal of ``Quu`` before the solves.  Returns an
        ``LqBackward``: ``K [B, T, nv, m]``, ``k [B, T, nv]`` -- the update is ``du = alpha k + K dx``, so an LQR gain is
        ``-K[:, 0]`` -- ``dV [B, 2]`` (the predicted change of cost is ``alpha dV[0] + alpha^2 dV[1]``) and ``status [B]`` int32:
        0, or ``t + 1`` of the first step whose ``Quu + mu I`` was not positive definite; that env's ``K``, ``k``, ``dV`` are then
        zeros -- raise its ``mu`` and call again.  Fields not in ``want`` are None (``status`` is always there).  Buffers kept per
        ``(body, want, T)`` and REUSED by the next call: clone what must last.  ValueError, before anything is launched, for
        everything the entry refuses and for tensors of the wrong shape, dtype or device."""
        fields = LqBackward._fields
        names = list(want) + ['status']
        if set(names) - set(fields):
            raise ValueError('want must name some of %r, got %r' % (fields[:3], want))
        body, _, nv = self._dyn_body(body)
        B, m = self.num_envs, 2 * nv
        dyn = [self._lq_rows(name, v, (nv, nv)) for name, v in (('A_q', A_q), ('A_v', A_v), ('Minv', Minv))]
        if any(t.dim() != dyn[0].dim() or t.shape[1] != dyn[0].shape[1] for t in dyn) or A_q.dim() < 3:
            raise ValueError('lq_backward_pass: A_q, A_v and Minv must all be [B, nv, nv] or all [B, P, nv, nv], got %s'
                             % ', '.join(str(tuple(v.shape)) for v in (A_q, A_v, Minv)))
        P = int(dyn[0].shape[1])
        T = int(horizon) if horizon is not None else P
        if P != 1 and P != T:
            raise ValueError('dg_world_lq_backward: P must be 1 or T = %d, got %d' % (T, P))
        cost = [None if v is None else self._lq_rows(name, v, tail) for name, v, tail in (('lxx', lxx, (m, m)), ('luu', luu, (nv, nv)), ('lx', lx, (m, )), ('lu', lu, (nv, )))]
        if cost[0] is None or cost[1] is None or lxx_T is None:
            raise ValueError('dg_world_lq_backward: lxx, luu and lxx_T are required')
        PC = max(int(t.shape[1]) for t in cost if t is not None)
        if PC != 1 and PC != T:
            raise ValueError("dg_world_lq_backward: the cost's P must be 1 or T = %d, got %d" % (T, PC))
        for name, t in zip(('lxx', 'luu', 'lx', 'lu'), cost):
            if t is not None and t.shape[1] not in (1, PC):
                raise ValueError('lq_backward_pass: %s has %d points per env, the other cost terms %d' % (name, t.shape[1], PC))
        cost = [None if t is None else t.expand((B, PC) + tuple(t.shape[2:])).contiguous() for t in cost]
        term = [None if v is None else self._lq_rows(name, v, tail) for name, v, tail in (('lxx_T', lxx_T, (m, m)), ('lx_T', lx_T, (m, )))]
        if any(t is not None and (t.shape[1] != 1 or v.dim() > len(t.shape) - 1) for t, v in zip(term, (lxx_T, lx_T))):
            raise ValueError('lq_backward_pass: lxx_T and lx_T are one per env ([m, m] / [m] or [B, ..])')
        term = [None if t is None else t.contiguous() for t in term]
        dyn = [t.contiguous() for t in dyn]
        if mu is not None:
            if not isinstance(mu, torch.Tensor):
                mu = torch.full((B, ), float(mu), dtype=torch.float32, device=self.device)
            mu = self._require('mu', mu, (B, ), torch.float32)
        key = ('lq_backward', body, T, tuple(f in names for f in fields))
        fresh = key not in self._dyn_out
        if fresh:
            shapes = {'K': (B, T, nv, m), 'k': (B, T, nv), 'dV': (B, 2), 'status': (B, )}
            self._dyn_out[key] = LqBackward(*[torch.zeros(shapes[f], dtype=torch.int32 if f == 'status' else torch.float32, device=self.device)
                                              if f in names else None for f in fields])
        out = self._dyn_out[key]
        try:
            self._dyn_check(self.lib.dg_world_lq_backward(self.handle, body, T, P, PC, int(substeps), float(dt), *[_ptr(t) for t in dyn], *[_ptr(t) for t in cost],
                                                          *[_ptr(t) for t in term], _ptr(mu), *[_ptr(t) for t in out], self._stream()))
        except ValueError:
            if fresh:   # a refused call keeps no buffers
                del self._dyn_out[key]
            raise
        return out

    def rollout_grid(self, K):
        """Diagnostic: the workgroups ``rollout_joint_dynamics`` launches for ``K`` samples per env (capped at the step's grid in the
        global-workspace modes, whose workspace is sized for that grid; the kernel strides over the rest)."""
        fn = self.lib.dg_debug_rollout_grid
        fn.restype, fn.argtypes = ctypes.c_int32, [_vp, ctypes.c_int32]
        n = fn(self.handle, int(K))
        if n < 0:
            raise ValueError(self.lib.dg_last_error().decode())
        return n

    # -- derivatives of the forward dynamics, and the forward dynamics as an autograd function ---------------------------------
    def _points_nv(self, name, v, nv):
        """``v`` for ``forward_dynamics_derivatives``: ``(tensor or None, P or None)``; ``[nv]`` and ``[B, nv]`` are one point per
        env, ``[B, P, nv]`` is P."""
        if v is None:
            return None, None
        if isinstance(v, torch.Tensor) and v.dim() == 3:
            return self._require(name, v, (self.num_envs, int(v.shape[1]), nv), torch.float32), int(v.shape[1])
        return self._rows_nv(name, v, nv), None

    def forward_dynamics_derivatives(self, body, q=None, qd=None, tau=None, joint_damping=False, want=('dqdd_dq', 'dqdd_dqd', 'dqdd_dtau')):
        """The derivatives of ``calculate_forward_dynamics`` for every env, at ``P`` points per env, in ONE launch
        (``dg_world_dynamics_derivatives``): what LQR, iLQR / DDP and an EKF linearise with.  Returns a ``DynamicsDerivatives``:
        ``qdd`` (the call's own ``calculate_forward_dynamics`` result), ``dqdd_dq``, ``dqdd_dqd`` (``[i][j]``: d qdd_i / d q_j, d qd_j),
        ``dqdd_dtau = M^-1``, ``dtau_dq``, ``dtau_dqd`` (the derivatives of the inverse dynamics at fixed ``qdd``, the second with
        the damping diagonal when ``joint_damping``; ``dqdd_dq = -M^-1 dtau_dq``) and ``singular`` int32.  Inputs ``[B, nv]`` or
        ``[nv]`` give matrices ``[B, nv, nv]``, ``qdd [B, nv]`` and ``singular [B]``; inputs ``[B, P, nv]`` (all given inputs must
        agree on ``P``; a ``[B, nv]`` or ``[nv]`` input cannot be mixed with them) give ``[B, P, nv, nv]``, ``[B, P, nv]`` and
        ``[B, P]``.  ``q`` / ``qd`` default to each env's current values, ``tau`` to zero, at every point.  The derivatives are
        analytic, first order only.  Fields not in ``want`` are None and cost nothing.  The env's per-env masses apply; the state
        is not written.  The tensors are buffers kept per ``(body, want, P)`` and REUSED by the next call: clone what must last.
        ValueError, before anything is launched, for everything the entry refuses and for tensors of the wrong shape, dtype or
        device."""
        fields = DynamicsDerivatives._fields
        names = list(want)
        if set(names) - set(fields):
            raise ValueError('want must name some of %r, got %r' % (fields, want))
        body, _, nv = self._dyn_body(body)
        ins = [self._points_nv(name, v, nv) for name, v in (('q', q), ('qd', qd), ('tau', tau))]
        given = [(name, P) for name, (t, P) in zip(('q', 'qd', 'tau'), ins) if t is not None]
        Ps = set(P for _, P in given)
        if len(Ps) > 1:
            raise ValueError('forward_dynamics_derivatives: the inputs must agree on the points per env, got %s'
                             % ', '.join('%s %s' % (name, 'one point [B, nv]' if P is None else 'P = %d' % P) for name, P in given))
        P = Ps.pop() if Ps else None
        B, n_pts = self.num_envs, 1 if P is None else P
        key = ('ddq', body, P, tuple(f in names for f in fields))
        fresh = False
        if key not in self._dyn_out:
            lead = (B, ) if P is None else (B, P)
            shapes = dict({f: lead + (nv, nv) for f in fields}, qdd=lead + (nv, ), singular=lead)
            self._dyn_out[key] = DynamicsDerivatives(*[torch.zeros(shapes[f], dtype=torch.int32 if f == 'singular' else torch.float32, device=self.device)
                                                       if f in names else None for f in fields])
            fresh = True
        out = self._dyn_out[key]
        try:
            self._dyn_check(self.lib.dg_world_dynamics_derivatives(self.handle, _ptr(self.state), body, n_pts, *[_ptr(t) for t, _ in ins], int(bool(joint_damping)),
                                                                   *[_ptr(t) for t in out], self._stream()))
        except ValueError:
            if fresh:   # a refused call keeps no buffers
                del self._dyn_out[key]
            raise
        return out

    # -- inertial parameters and the regressor of the inverse dynamics ---------------------------------------------------------
    def inertial_parameters(self, body, nominal=False):
        """The inertial parameters of the body's links for every env (``dg_world_inertial_parameters``): ``[B, nv, 10]``, per link
        ``[m, m cx, m cy, m cz, Ixx, Ixy, Ixz, Iyy, Iyz, Izz]`` in the link's own frame, ``c`` the centre of mass and ``I`` the inertia
        about the link-frame origin; a link is a movable joint's child link with everything fixed to it merged.  The env's mass scale
        (``dynamics_randomizer``) multiplies all ten -- the TRUE parameters, privileged information on the device; ``nominal=True``
        gives the scene's unscaled values.  ``calculate_inverse_dynamics(q, qd, qdd) = Y(q, qd, qdd) theta`` with
        ``inverse_dynamics_regressor``'s ``Y``.  The tensor is a buffer kept per ``(body, nominal)`` and REUSED: clone what must last."""
        body, _, nv = self._dyn_body(body)
        theta = self._dyn_buf('theta_nominal' if nominal else 'theta', body, self.num_envs, nv, 10)
        self._dyn_check(self.lib.dg_world_inertial_parameters(self.handle, _ptr(self.state), body, int(bool(nominal)), _ptr(theta), self._stream()))
        return theta

    def inverse_dynamics_regressor(self, body, q=None, qd=None, qdd=None, qd_ref=None, theta=None, s=None, want=('Y', )):
        """The regressor of the inverse dynamics for every env, at ``P`` points per env, in ONE launch (``dg_world_id_regressor``):
        ``tau = Y(q, qd, qdd) theta`` with ``theta`` as ``inertial_parameters`` orders it.  With ``qd_ref`` it is the Slotine-Li form
        ``Y theta = M qdd + C(q, qd) qd_ref - G`` (``Mdot - 2 C`` skew-symmetric).  Returns a ``DynamicsRegressor``: ``Y``
        ``[B, (P,) nv, 10 nv]``; ``tau = Y theta`` ``[B, (P,) nv]`` and ``grad = Y^T s`` ``[B, (P,) 10 nv]``, both formed without ``Y``
        in O(nv).  ``q``, ``qd``, ``qdd``, ``qd_ref`` and ``s`` are ``[nv]``, ``[B, nv]`` or ``[B, P, nv]`` (all given inputs must
        agree on ``P``); ``q`` / ``qd`` default to each env's current values, ``qdd`` to zero, ``qd_ref`` to ``qd``.  ``theta`` is
        ``[10 nv]``, ``[B, 10 nv]`` or ``[B, nv, 10]``: per env, never per point -- the caller's estimate; the env's own masses do not
        enter.  ``'tau'`` in ``want`` needs ``theta`` and ``'grad'`` needs ``s``.  Fields not in ``want`` are None and cost nothing.
        The tensors are buffers kept per ``(body, want, P)`` and REUSED by the next call: clone what must last.  ValueError, before
        anything is launched, for everything the entry refuses and for tensors of the wrong shape, dtype or device."""
        fields = DynamicsRegressor._fields
        names = list(want)
        if not names or set(names) - set(fields):
            raise ValueError('want must name some of %r, got %r' % (fields, want))
        if 'tau' in names and theta is None:
            raise ValueError("inverse_dynamics_regressor: 'tau' in want needs theta")
        if 'grad' in names and s is None:
            raise ValueError("inverse_dynamics_regressor: 'grad' in want needs s")
        body, _, nv = self._dyn_body(body)
        args = ('q', 'qd', 'qdd', 'qd_ref', 's')
        ins = [self._points_nv(name, v, nv) for name, v in zip(args, (q, qd, qdd, qd_ref, s))]
        given = [(name, P) for name, (t, P) in zip(args, ins) if t is not None]
        Ps = set(P for _, P in given)
        if len(Ps) > 1:
            raise ValueError('inverse_dynamics_regressor: the inputs must agree on the points per env, got %s'
                             % ', '.join('%s %s' % (name, 'one point [B, nv]' if P is None else 'P = %d' % P) for name, P in given))
        P = Ps.pop() if Ps else None
        B, n_pts = self.num_envs, 1 if P is None else P
        if theta is not None:
            if isinstance(theta, torch.Tensor) and theta.dim() == 1:
                theta = self._rows_nv('theta', theta, 10 * nv)
            elif isinstance(theta, torch.Tensor) and theta.dim() == 3:
                theta = self._require('theta', theta, (B, nv, 10), torch.float32)
            else:
                theta = self._require('theta', theta, (B, 10 * nv), torch.float32)
        key = ('regq', body, P, tuple(f in names for f in fields))
        if key not in self._dyn_out:
            lead = (B, ) if P is None else (B, P)
            shapes = {'Y': lead + (nv, 10 * nv), 'tau': lead + (nv, ), 'grad': lead + (10 * nv, )}
            self._dyn_out[key] = DynamicsRegressor(*[torch.zeros(shapes[f], dtype=torch.float32, device=self.device) if f in names else None for f in fields])
        out = self._dyn_out[key]
        (q, _), (qd, _), (qdd, _), (qd_ref, _), (s, _) = ins
        self._dyn_check(self.lib.dg_world_id_regressor(self.handle, _ptr(self.state), body, n_pts, _ptr(q), _ptr(qd), _ptr(qdd), _ptr(qd_ref),
                                                       _ptr(theta if out.tau is not None else None), _ptr(s if out.grad is not None else None),
                                                       _ptr(out.Y), _ptr(out.tau), _ptr(out.grad), self._stream()))
        return out

    def forward_dynamics_fn(self, body, joint_damping=False):
        """``f(q, qd, tau) -> qdd``: ``calculate_forward_dynamics`` as a ``torch.autograd.Function``, so that ``loss.backward()`` goes
        through the body's rigid-body model.  ``q``, ``qd``, ``tau`` are ``[B, nv]`` or ``[B, P, nv]`` float32 tensors on this
        device.  Forward is ONE ``forward_dynamics_derivatives`` launch: it returns a fresh ``qdd`` and saves clones of the three
        ``dqdd_*`` matrices; backward is three batched products, ``g_q = dqdd_dq^T g``, ``g_qd = dqdd_dqd^T g``,
        ``g_tau = dqdd_dtau^T g``, only for the inputs that need a gradient (the others' matrices are not computed).  FIRST derivatives only:
        the saved matrices are constants of the graph, and ``backward`` is marked ``once_differentiable``, so asking for a gradient of a
        gradient through ``f`` raises instead of returning zero."""
        sim = self
        damping = bool(joint_damping)

        class ForwardDynamics(torch.autograd.Function):
            @staticmethod
            def forward(ctx, q, qd, tau):
                need = tuple(ctx.needs_input_grad[:3])   # only the matrices backward will read are computed, cloned and saved
                d = sim.forward_dynamics_derivatives(body, q.detach().contiguous(), qd.detach().contiguous(), tau.detach().contiguous(), damping,
                                                     want=('qdd', ) + tuple(f for f, n in zip(('dqdd_dq', 'dqdd_dqd', 'dqdd_dtau'), need) if n))
                ctx.need = need
                ctx.save_for_backward(*[m.clone() for m, n in zip((d.dqdd_dq, d.dqdd_dqd, d.dqdd_dtau), need) if n])
                return d.qdd.clone()

            @staticmethod
            @torch.autograd.function.once_differentiable
            def backward(ctx, g):
                mats = iter(ctx.saved_tensors)
                g = g.contiguous().unsqueeze(-2)   # [.., 1, nv] x [.., nv, nv] -> g^T J = (J^T g)^T
                return tuple(torch.matmul(g, next(mats)).squeeze(-2) if n else None for n in ctx.need)

        return ForwardDynamics.apply

    # -- the second half of p.getJointState(s): jointReactionForces, appliedJointMotorTorque ------------------------------------
    def joint_reaction_forces(self, body, joints=None):
        """``p.getJointStates(uid, joints)[..][2]`` after ``p.enableJointForceTorqueSensor`` for every env at once, in ONE launch:
        ``[B, n, 6]``, row k ``[Fx Fy Fz Mx My Mz]`` of joint ``joints[k]`` -- the force and the torque the PARENT side exerts on
        the CHILD side through the joint, expressed in the inertial frame of the joint's child link, the torque about that frame's
        origin: exactly what the compiled ``force_torque_sensor`` reports.  ``body`` is a Model's ``uid``; ``joints`` a list of up
        to 16 of what ``Model.get_frame_id`` returns, fixed or movable (None: every movable joint of the body, if there are at most
        16).  The scene must keep the body's velocities at the start of the last substep: ``builder.enable_joint_force_torque(uid)``
        in an addon's ``compile()`` (``joint_wrench_sensor`` does it), or a compiled ``force_torque_sensor`` on the model.

        The child side is the rigid cluster of URDF links behind the joint (the whole moving link when the joint is movable) plus
        every moving link hanging off it.  The reading is Newton-Euler over it with the accelerations ``(v_now - v_prev) / h`` of
        the last substep and gravity taken off, minus the contact forces on child-side shapes; a contact counts when exactly one of
        its two shapes is on the child side, and its arm is the contact POINT -- the midpoint of ``contact_points``' ``pos_a`` and
        ``pos_b`` -- as in the compiled sensor, NOT the surface point ``net_contact_forces`` uses.  Motors, applied joint torques
        and external wrenches are no terms of their own: they show through the motion.

        Staleness as ``contact_forces``: the contact geometry is that of the CURRENT state, the impulses those of the LAST substep
        for the contact with the same key, 0 for a new one; the compiled sensor reads the last substep's own list, so the two
        agree to rounding where nothing touches and at rest and differ by one substep of motion while contacts move.  Nothing saves
        velocities on a teleport: after ``reset_joint_state``, ``reset_base_state`` or a ``set_state`` that changes a velocity the
        next reading carries the jump ``(v_new - v_prev) / h``; the next step clears it.  After ``reset()`` the accelerations are
        zero and the cache is empty: the plain gravity load.  The state is not written.

        ValueError: a body without saved velocities, a frozen body or an attached child model, a joint the body does not have, not
        1 .. 16 joints.  RuntimeError: a world with contact pairs that keeps no contact impulse cache (``warmstart`` and
        ``warmstart_friction`` both 0).

        The result is a buffer kept per ``(body, joints)`` and REUSED by the next call with the same arguments: clone what must last."""
        key = (int(body), None if joints is None else tuple(int(j) for j in joints))
        if key not in self._joint_wrench_out:
            b, js, arr = joint_wrench_selectors(self.layout, body, joints)
            self._joint_wrench_out[key] = (b, arr, torch.empty((self.num_envs, len(js), 6), dtype=torch.float32, device=self.device))
        b, arr, out = self._joint_wrench_out[key]
        self._dyn_check(self.lib.dg_world_joint_wrench(self.handle, _ptr(self.state), b, arr, len(arr), _ptr(out), self._stream()))
        return out

    def joint_motor_torques(self, body):
        """``p.getJointStates(uid, joints)[..][3]`` (appliedJointMotorTorque) for every env: ``[B, nv]``, the motor torque applied to
        each joint during the last solver pass -- the ``effort`` of ``joint_state_sensor``, what ``electricity_cost`` multiplies with
        the joint rates.  Any body with joints, fixed or floating base; the alias uid of a merged child gives the PARENT's ``nv``,
        like ``joint_states``.  The result is a buffer kept per body and REUSED by the next call: clone what must last."""
        body = self.layout.resolve_frame(body, -1)[0]
        if not 0 <= body < self.layout.n_bodies:
            raise ValueError('dg_world_joint_efforts: body %d out of range' % body)
        nv = int(self.layout.body_n_links[body])
        if nv < 1:
            raise ValueError('dg_world_joint_efforts: body %d has no joints' % body)
        out = self._dyn_buf('effort', body, self.num_envs, nv)
        self._dyn_check(self.lib.dg_world_joint_efforts(self.handle, _ptr(self.state), body, _ptr(out), self._stream()))
        return out

    # -- how links accelerate, and what an IMU on one reads (no pybullet counterpart) --------------------------------------------
    def link_accelerations(self, body, frames=None, local_pos=None, local_orn=None, com=False):
        """How links of ``body`` ACCELERATE and what an accelerometer and a gyro mounted on them read, for every env at once, in ONE
        launch.  A named tuple ``(lin_acc, ang_acc, specific_force, ang_vel, gravity)``, each a ``[B, n, 3]`` view of one
        ``[B, n, 15]`` buffer.  ``body`` is a Model's ``uid``; ``frames`` up to 16 of what ``Model.get_frame_id`` returns, -1 the base
        (None: the base alone); ``com`` False: the URDF link frame ``camera`` and ``lidar`` mount on, True: the link's inertial frame,
        as ``link_states``; ``local_pos`` ``[n, 3]`` and ``local_orn`` ``[n, 4]`` xyzw a mount pose in that frame (one vector applies
        to every selector; default identity).

        With S the sensor frame (world rotation ``R_s``, origin ``p_s``), L the moving link it is rigidly attached to, ``w, alpha,
        a`` that link's angular velocity and accelerations -- ``(v_now - v_prev) / h`` over the LAST SUBSTEP, as
        ``joint_reaction_forces`` forms them -- ``r = p_s - p_L`` and ``g`` the scene's gravity:

        * ``lin_acc`` = ``a + alpha x r + w x (w x r)`` and ``ang_acc`` = ``alpha``, world axes;
        * ``specific_force`` = ``R_s^T (lin_acc - g)``: what an accelerometer reads, ``(0, 0, +|g|)`` at rest and level;
        * ``ang_vel`` = ``R_s^T w``: what a gyro reads;
        * ``gravity`` = ``R_s^T g / |g|`` (zeros when ``g = 0``): the projected gravity direction.

        No contact term and no narrow phase: contact, motor and external forces show through the motion.  The scene must keep the
        body's velocities at the start of the last substep: ``builder.enable_joint_force_torque(uid)`` in an addon's ``compile()``
        (``imu_sensor`` does it), or a compiled ``force_torque_sensor`` on the model.  Nothing saves velocities on a teleport: after
        ``reset_joint_state``, ``reset_base_state`` or a ``set_state`` that changes a velocity the next reading carries the jump
        ``(v_new - v_prev) / h``; the next step clears it.  After ``reset()`` the accelerations are zero and ``specific_force`` is
        ``-R_s^T g``.  The state is not written.  Sensor noise and bias are the caller's to add to the tensors.

        ValueError, before any launch: a body without saved velocities (a fixed base without joints keeps none: its reading is the
        constant ``-g``), a frozen body or an attached child model, a frame the body does not have, not 1 .. 16 frames, a mount
        quaternion of zero norm.

        The buffer is kept per ``n`` and REUSED by the next call with as many frames: clone what must last."""
        key = (int(body), None if frames is None else tuple(frames), _mount_key(local_pos), _mount_key(local_orn), bool(com))
        hit = self._link_accel_sel.get(key)
        if hit is None:
            b, arr = link_accel_selectors(self.layout, body, frames, local_pos, local_orn, com)
            n = len(arr)
            if n not in self._link_accel_out:
                out = torch.empty((self.num_envs, n, LA_STRIDE), dtype=torch.float32, device=self.device)
                views = LinkAccelerations(*(out[:, :, k:k + 3] for k in (LA_LIN_ACC, LA_ANG_ACC, LA_SPECIFIC_FORCE, LA_ANG_VEL, LA_GRAVITY)))
                self._link_accel_out[n] = (_ptr(out), views)
            hit = self._link_accel_sel[key] = (b, arr, n) + self._link_accel_out[n]
        b, arr, n, out_ptr, views = hit
        self._dyn_check(self.lib.dg_world_link_accelerations(self.handle, _ptr(self.state), b, arr, n, out_ptr, self._stream()))
        return views

    # -- batched p.calculateInverseKinematics / POSITION_CONTROL, VELOCITY_CONTROL targets / p.resetJointState ----------------
    # The position-level half of the same contract (reference diy_gym/addons/controllers/ik_controller.py:47-80): same bodies,
    # same conventions, same reused output buffers as the dynamics queries above.
    def _ik_lists(self, nv, rest, lower, upper, ranges):
        """The four null-space lists as one device ``[4, nv]`` tensor in the order rest, lower, upper, range -- uploaded once per
        distinct value and kept; None when none is given.  ValueError for a partial set or a list of another length."""
        given = [v is not None for v in (rest, lower, upper, ranges)]
        if not any(given):
            return None
        if not all(given):
            raise ValueError('the null-space term takes all four of lower, upper, ranges, rest; got only %s' %
                             ', '.join(n for n, g in zip(('rest', 'lower', 'upper', 'ranges'), given) if g))
        rows = []
        for name, v in (('rest', rest), ('lower', lower), ('upper', upper), ('ranges', ranges)):
            row = tuple(float(x) for x in (v.tolist() if hasattr(v, 'tolist') else v))
            if len(row) != nv:
                raise ValueError('%s must have %d entries (one per joint of the body), got %d' % (name, nv, len(row)))
            rows.append(row)
        key = tuple(rows)
        if key not in self._ik_list_cache:
            self._ik_list_cache[key] = torch.tensor(rows, dtype=torch.float32, device=self.device)
        return self._ik_list_cache[key]

    def _joint_mask(self, joints, nv):
        """The bit mask of ``joints`` (indices of the body's joints; None: all of them)."""
        if joints is None:
            return ctypes.c_uint64(0xFFFFFFFFFFFFFFFF)
        m = 0
        for j in joints:
            if not 0 <= int(j) < min(nv, 64):
                raise ValueError('joint %d out of range (the body has %d joints; a joint list reaches the first 64)' % (int(j), nv))
            m |= 1 << int(j)
        return ctypes.c_uint64(m)

    def calculate_inverse_kinematics(self, body, frame, target_pos, target_orn=None, lower=None, upper=None, ranges=None, rest=None, q0=None,
                                     return_iters=False):
        """``p.calculateInverseKinematics(uid, linkIndex, targetPosition, targetOrientation, lowerLimits, upperLimits, jointRanges,
        restPoses)`` for every env: ``[B, nv]`` joint positions, or ``(q, iters)`` with ``return_iters`` (``iters``: int32 ``[B]``,
        the iterations each env ran before its position error fell below the world's ``ik_residual``).  The recursion, its
        iteration count, damping, clamp and gains are those of the world's ``ik_controller`` op (the engine parameters ``ik_*``).
        ``frame`` is the index ``Model.get_frame_id`` returns (>= 0); the target is the pose of that link's INERTIAL frame -- what
        ``frame_state(uid, frame, com=True)`` reports -- as ``[B, 3]`` (or one 3-vector) and a unit quaternion xyzw ``[B, 4]`` (or one;
        None: position only).  ``lower, upper, ranges, rest``: host sequences of ``nv`` numbers; the null-space term is on when all
        four are given, a partial set raises ValueError.  ``q0``: where the iteration starts (default: each env's current joint
        positions).  The state is not written."""
        if int(frame) < 0:
            raise ValueError('frame must be a frame id >= 0, got %d' % int(frame))
        body, frame, nv = self._dyn_body(body, frame)
        lists = self._ik_lists(nv, rest, lower, upper, ranges)
        tp = self._rows_k('target_pos', target_pos, 3, body)
        if tp is None:
            raise ValueError('target_pos must be a torch.Tensor, got None')
        to = self._rows_k('target_orn', target_orn, 4, body)
        q0 = self._rows_nv('q0', q0, nv)
        q = self._dyn_buf('ik_q', body, self.num_envs, nv)
        key = ('ik_iters', body)
        if return_iters and key not in self._dyn_out:
            self._dyn_out[key] = torch.zeros((self.num_envs, ), dtype=torch.int32, device=self.device)
        it = self._dyn_out[key] if return_iters else None
        self._dyn_check(self.lib.dg_world_inverse_kinematics(self.handle, _ptr(self.state), body, frame, _ptr(tp), _ptr(to), _ptr(lists), _ptr(q0), _ptr(q),
                                                             _ptr(it), self._stream()))
        return (q, it) if return_iters else q

    def _rows_k(self, name, v, k, body):
        """``v`` (float32, this device) as a contiguous ``[num_envs, k]`` tensor: one ``[k]`` vector for every env, or one per env."""
        if v is None:
            return None
        if isinstance(v, torch.Tensor) and v.dim() == 1:
            buf = self._dyn_buf('in_' + name, body, self.num_envs, k)
            buf.copy_(self._require(name, v, (k, ), torch.float32).reshape(1, k))
            return buf
        return self._require(name, v, (self.num_envs, k), torch.float32)

    def set_joint_motor_targets(self, body, positions=None, velocities=None, joints=None):
        """``p.setJointMotorControlArray(uid, joints, p.POSITION_CONTROL, targetPositions=positions[, targetVelocities=velocities])``
        or, with ``velocities`` alone, ``(uid, joints, p.VELOCITY_CONTROL, targetVelocities=velocities)`` for every env.  Both are
        ``[B, nv]`` (or ``[nv]``) over ALL the body's joints; ``joints`` (indices of the body's joints, default all) selects the
        columns that are written.  The position form sets the velocity target to ``velocities`` or 0, the velocity form sets the
        position target to 0.  Targets persist until overwritten; gains and force limits are the motor table's (``set_motor_cfg``)."""
        body, _, nv = self._dyn_body(body)
        if positions is None and velocities is None:
            raise ValueError('give positions, velocities or both')
        pos, vel = self._rows_nv('positions', positions, nv), self._rows_nv('velocities', velocities, nv)
        self._dyn_check(self.lib.dg_world_set_joint_targets(self.handle, _ptr(self.state), body, self._joint_mask(joints, nv), _ptr(pos), _ptr(vel),
                                                            self._stream()))

    def reset_joint_state(self, body, q, qd=None, joints=None, mask=None):
        """``p.resetJointState(uid, joint, q, qd)`` for the joints ``joints`` (default all) of the envs ``mask`` selects (as for
        ``reset``; default all): ``q`` and ``qd`` are ``[B, nv]`` (or ``[nv]``) over ALL the body's joints, ``qd`` defaults to zero.
        Motor targets are left alone, as in pybullet; the reset envs' contact impulse cache is emptied.  Observations are refreshed by
        the next ``observe()`` or ``step()``."""
        body, _, nv = self._dyn_body(body)
        if q is None:
            raise ValueError('q must be a torch.Tensor, got None')
        q, qd = self._rows_nv('q', q, nv), self._rows_nv('qd', qd, nv)
        self._dyn_check(self.lib.dg_world_reset_joint_state(self.handle, _ptr(self.state), body, self._joint_mask(joints, nv), _ptr(q), _ptr(qd),
                                                            _ptr(self._env_mask(mask)), self._stream()))

    # -- batched p.getContactPoints ---------------------------------------------------------------------------------------
    def _contact_filter(self, side, body, link):
        """``(body index, link index)`` of one side's filter as ``dg_world_contacts`` takes it; ValueError for what it would refuse."""
        if body is None:
            if link is not None:
                raise ValueError('link_%s given without body_%s' % (side, side))
            return CONTACT_ANY, CONTACT_ANY
        body = int(body)
        if body in self.layout.aliases:   # a merged child: its shapes carry the parent's uid (and their own URDF link index)
            body = self.layout.aliases[body][0]
        if not 0 <= body < self.layout.n_bodies:
            raise ValueError('body_%s %d is not a model of this scene' % (side, body))
        if link is None:
            return body, CONTACT_ANY
        if int(link) < -1:
            raise ValueError('link_%s must be a frame id (-1: the base), got %d' % (side, int(link)))
        return body, int(link)

    def contact_points(self, body_a=None, body_b=None, link_a=None, link_b=None, want=('id', 'pos', 'normal', 'distance', 'force')):
        """``p.getContactPoints(bodyA, bodyB, linkIndexA, linkIndexB)`` for every env at once.  Returns ``ContactPoints(count, id_a,
        id_b, pos_a, pos_b, normal, distance, normal_force)`` with C = the scene's ``max_contacts``: ``count [B]`` int32, ``id_a``,
        ``id_b`` ``[B, C]`` int32 ``uid + ((link + 1) << 24)`` (the ids of the camera's segmentation mask and of ``ray_test_batch``),
        ``pos_a``, ``pos_b`` ``[B, C, 3]`` world points on the two surfaces, ``normal [B, C, 3]`` the unit normal on B pointing
        towards A, ``distance [B, C]`` (negative: penetration) and ``normal_force [B, C]`` in newtons; the groups ``want`` (any of
        'id', 'pos', 'normal', 'distance', 'force') leaves out are None.  Rows are in the order of the narrow phase's pairs; behind an
        env's ``count`` the ids are -1 and everything else 0, so ``normal_force.sum(1)`` needs no mask.

        ``body_*`` are Models' ``uid``, ``link_*`` what ``Model.get_frame_id`` returns (-1: the base); None is no filter, a link
        without its body raises.  With ``body_a`` alone every row has that body as side A (sides swapped and the normal negated
        where the narrow phase had it as B); with both, either orientation matches and is reported as (a, b).  The alias uid of a
        child model merged rigidly into its parent is matched by the id the camera reports for the child's shapes: the PARENT's
        uid, with the link index the shape has in the child's own URDF -- so an alias without a link selects the whole merged body.  A link is accepted
        when a shape of the body carries it or the body has such a frame; a child's link index can coincide with one of the
        parent's own, and then both match.

        The geometry is that of the CURRENT state; the force is what the solver applied in the LAST substep to the contact with the
        same key -- 0 for a contact that is new since then or whose feature changed, and for every contact after
        ``reset_joint_state`` until the next step (``dg_world_contacts`` has the rule in full).  'force' needs the contact impulse
        cache: a world created with ``warmstart`` and ``warmstart_friction`` both 0 raises RuntimeError when asked for it.

        The tensors are views of buffers kept per ``want`` and REUSED by the next call: clone what must last."""
        groups = ('id', 'pos', 'normal', 'distance', 'force')
        unknown = set(want) - set(groups)
        if unknown:
            raise ValueError("want may name 'id', 'pos', 'normal', 'distance', 'force', got %r" % (want, ))
        ba, la = self._contact_filter('a', body_a, link_a)
        bb, lb = self._contact_filter('b', body_b, link_b)
        B, C = self.num_envs, int(self.layout.max_contacts)
        Cs = max(C, 1)   # (a scene without candidate pairs has C = 0: the buffers still exist, the views are empty)
        need_geom = any(g in want for g in ('pos', 'normal', 'distance'))
        key = ('id' in want, need_geom, 'force' in want)
        if key not in self._contact_out:
            self._contact_out[key] = (torch.zeros((B, ), dtype=torch.int32, device=self.device),
                                      torch.empty((B, Cs, 2), dtype=torch.int32, device=self.device) if key[0] else None,
                                      torch.empty((B, Cs, 10), dtype=torch.float32, device=self.device) if key[1] else None,
                                      torch.empty((B, Cs), dtype=torch.float32, device=self.device) if key[2] else None)
        count, ids, geom, force = self._contact_out[key]
        self._dyn_check(self.lib.dg_world_contacts(self.handle, _ptr(self.state), ba, la, bb, lb, _ptr(count), _ptr(ids), _ptr(geom), _ptr(force),
                                                   self._stream()))
        pos, nrm, dist = 'pos' in want, 'normal' in want, 'distance' in want
        return ContactPoints(count, None if ids is None else ids[:, :C, 0], None if ids is None else ids[:, :C, 1],
                             geom[:, :C, 0:3] if pos else None, geom[:, :C, 3:6] if pos else None, geom[:, :C, 6:9] if nrm else None,
                             geom[:, :C, 9] if dist else None, None if force is None else force[:, :C])

    # -- contact forces in full: lateral friction, per-link net wrench -------------------------------------------------------
    def contact_forces(self, body_a=None, body_b=None, link_a=None, link_b=None, want=('id', 'force')):
        """The contact forces ``contact_points`` leaves out, for every env at once.  Returns ``ContactForces(count, id_a, id_b, normal,
        normal_force, lateral_friction1, lateral_dir1, lateral_friction2, lateral_dir2, force_on_a)``: rows, ``count``, ids, filters
        and side swapping are exactly ``contact_points``' (same state, same filters: the same rows in the same order);
        ``normal [B, C, 3]`` and ``normal_force [B, C]`` are its bits; ``lateral_friction1/2 [B, C]`` are the signed friction forces
        in newtons along the unit tangents ``lateral_dir1/2 [B, C, 3]`` (pybullet's lateralFriction1/2, lateralFrictionDir1/2: the
        basis the solver's friction rows were built with), and ``force_on_a [B, C, 3]`` is the total force the contact applies to
        side A in world axes (side B receives its negative)::

            force_on_a = normal_force * normal + lateral_friction1 * lateral_dir1 + lateral_friction2 * lateral_dir2

        Where the filter swaps the sides the normal and both tangents are negated and the scalars kept, so ``(X, Y)`` and ``(Y, X)``
        report exactly opposite forces.  ``want`` names the groups 'id' and 'force' (everything but the ids); what it leaves out is
        None.  Behind an env's ``count`` the ids are -1 and everything else 0.

        Staleness as ``contact_points``: geometry and tangents are those of the CURRENT state, the three impulses those of the LAST
        substep for the contact with the same key, 0 for a new one (``dg_world_contact_forces`` has the rule in full).  A world
        created with ``warmstart`` and ``warmstart_friction`` both 0 keeps no impulses: RuntimeError.

        The tensors are views of buffers kept per ``want`` and REUSED by the next call: clone what must last."""
        unknown = set(want) - {'id', 'force'}
        if unknown:
            raise ValueError("want may name 'id', 'force', got %r" % (want, ))
        ba, la = self._contact_filter('a', body_a, link_a)
        bb, lb = self._contact_filter('b', body_b, link_b)
        B, C = self.num_envs, int(self.layout.max_contacts)
        Cs = max(C, 1)
        key = ('id' in want, 'force' in want)
        if key not in self._contact_force_out:
            self._contact_force_out[key] = (torch.zeros((B, ), dtype=torch.int32, device=self.device),
                                            torch.empty((B, Cs, 2), dtype=torch.int32, device=self.device) if key[0] else None,
                                            torch.empty((B, Cs, 15), dtype=torch.float32, device=self.device) if key[1] else None)
        count, ids, f = self._contact_force_out[key]
        self._dyn_check(self.lib.dg_world_contact_forces(self.handle, _ptr(self.state), ba, la, bb, lb, _ptr(count), _ptr(ids), _ptr(f), self._stream()))
        if f is None:
            return ContactForces(count, ids[:, :C, 0] if key[0] else None, ids[:, :C, 1] if key[0] else None, None, None, None, None, None, None, None)
        return ContactForces(count, None if ids is None else ids[:, :C, 0], None if ids is None else ids[:, :C, 1], f[:, :C, 0:3], f[:, :C, 3],
                             f[:, :C, 4], f[:, :C, 5:8], f[:, :C, 8], f[:, :C, 9:12], f[:, :C, 12:15])

    def _body_n_frames(self, body):
        """Frames of a body (the merged children's included), from the scene blob's frame table."""
        K = _scene_constants()
        I = self.layout.I
        n, off = int(I[K.H_N_FRAMES]), int(I[K.H_OFF_FRAME_I])
        return int((I[off:off + n * K.FI_STRIDE].reshape(n, K.FI_STRIDE)[:, K.FI_BODY] == body).sum())

    def _net_contact_links(self, body, links):
        """``(body index, [link index or CONTACT_ANY, ...])`` of net_contact_forces' selectors as ``dg_world_net_contact_wrench`` takes
        them; ValueError for what it would refuse."""
        body, _ = self._contact_filter('', body, None)
        if body == CONTACT_ANY:
            raise ValueError('net_contact_forces needs a body')
        links = [None] if links is None else list(links)
        if not 1 <= len(links) <= CONTACT_MAX_LINKS:
            raise ValueError('net_contact_forces takes 1 .. %d links, got %d' % (CONTACT_MAX_LINKS, len(links)))
        out = []
        for l in links:
            if l is None:
                out.append(CONTACT_ANY)
                continue
            l = int(l)
            if not -1 <= l < self._body_n_frames(body):
                raise ValueError('link %d is not a frame of body %d (None: the whole body, -1: the base)' % (l, body))
            out.append(l)
        return body, out

    def net_contact_forces(self, body, links=None, body_b=None, link_b=None, want=('force', 'torque', 'count')):
        """The net contact wrench on links of one body, for every env at once, in ONE launch: ``(force [B, n, 3], torque [B, n, 3],
        count [B, n])``.  ``body`` is a Model's ``uid``; ``links`` a list of up to 16 of what ``Model.get_frame_id`` returns (-1:
        the base), each selecting the contacts that have THAT link of the body on a side (for the alias uid of a merged child: frame
        ids of the PARENT's merged body); ``None`` in the list -- or ``links=None``,
        one row -- selects the whole body.  ``body_b`` / ``link_b`` optionally restrict the other side, as in ``contact_points``.

        ``force`` is the sum of the forces the selected contacts apply to this body (normal and friction), world axes, in newtons;
        ``torque`` the sum of their moments about the origin of the link's INERTIAL frame -- the point ``frame_state(body, link,
        com=True)`` reports; the base's for ``None`` -- with the contact's surface point on this body as the arm; ``count`` int32
        the number of contacts summed.  What ``want`` leaves out is None.  A link selector must be a frame of the body: the shapes of
        a merged child model carry the child's own link indices and are reached through the whole-body row and through
        ``contact_forces``.  Staleness and the impulse cache as ``contact_forces``.

        The tensors are views of buffers kept per number of links and REUSED by the next call: clone what must last."""
        unknown = set(want) - {'force', 'torque', 'count'}
        if unknown:
            raise ValueError("want may name 'force', 'torque', 'count', got %r" % (want, ))
        body, links = self._net_contact_links(body, links)
        bb, lb = self._contact_filter('b', body_b, link_b)
        B, n = self.num_envs, len(links)
        key = (n, 'count' in want)
        if key not in self._net_contact_out:
            self._net_contact_out[key] = (torch.empty((B, n, 6), dtype=torch.float32, device=self.device),
                                          torch.empty((B, n), dtype=torch.int32, device=self.device) if key[1] else None)
        wrench, cnt = self._net_contact_out[key]
        arr = (ctypes.c_int32 * n)(*links)
        self._dyn_check(self.lib.dg_world_net_contact_wrench(self.handle, _ptr(self.state), body, arr, n, bb, lb, _ptr(wrench), _ptr(cnt), self._stream()))
        return (wrench[:, :, 0:3] if 'force' in want else None, wrench[:, :, 3:6] if 'torque' in want else None, cnt)

    # -- batched p.getClosestPoints ---------------------------------------------------------------------------------------
    def closest_points(self, body_a, body_b=None, distance=0.1, link_a=None, link_b=None, max_points=None,
                       want=('id', 'pos', 'normal', 'distance', 'nearest')):
        """``p.getClosestPoints(bodyA, bodyB, distance, linkIndexA, linkIndexB)`` for every env at once: every pair of collision
        shapes of the two sides that is nearer than ``distance`` (penetrating pairs always), the pairs the step never tests because
        static pruning removed them included.  Returns ``ClosestPoints(count, id_a, id_b, pos_a, pos_b, normal, distance,
        nearest_id_a, nearest_id_b, nearest_pos_a, nearest_pos_b, nearest_normal, nearest_distance)``: ``count [B]`` int32 (pairs
        found, whether or not they fit in K: ``count > K`` means the rows were truncated), ``id_a``, ``id_b`` ``[B, K]`` int32 ids
        as ``contact_points``, ``pos_a``, ``pos_b``, ``normal`` ``[B, K, 3]`` (the normal on B pointing towards A), ``distance
        [B, K]``; rows in (shape of A, shape of B) order, ids -1 and zeros behind them.  ``nearest_*`` (``[B]``, ``[B, 3]``) is the
        pair of smallest distance over ALL pairs found, independent of K; with nothing within ``distance`` its ids are -1, positions
        and normal 0 and ``nearest_distance == distance``, so it serves as an observation as it is.  The groups ``want`` (any of
        'id', 'pos', 'normal', 'distance', 'nearest') leaves out are None.

        ``body_a`` (required) and ``body_b`` are Models' ``uid`` (None: any other body), ``link_*`` what ``Model.get_frame_id``
        returns (-1: the base); the alias uid of a merged child is matched as in ``contact_points``.  ``body_a`` is always side A.
        ``max_points`` K: None = the number of candidate shape pairs of the filter, at most 64.  Each pair is measured in the step's
        own model of it (``dg_world_closest``); box against box and two bodies that both cannot move are never pairs.  There is no
        force.  Argument errors raise ValueError.

        The tensors are views of buffers kept per ``(want, K)`` and REUSED by the next call: clone what must last."""
        groups = ('id', 'pos', 'normal', 'distance', 'nearest')
        unknown = set(want) - set(groups)
        if unknown:
            raise ValueError("want may name 'id', 'pos', 'normal', 'distance', 'nearest', got %r" % (want, ))
        if body_a is None:
            raise ValueError('body_a is required (body_b may be None: any other body)')
        ba, la = self._contact_filter('a', body_a, link_a)
        bb, lb = self._contact_filter('b', body_b, link_b)
        distance = float(distance)
        if not np.isfinite(distance) or distance < 0.0:
            raise ValueError('distance must be finite and >= 0, got %r' % (distance, ))
        if max_points is None:
            key = (ba, la, bb, lb)
            if key not in self._closest_k:
                self._closest_k[key] = min(len(closest_candidate_pairs(self.layout, ba, la, bb, lb)), CLOSEST_MAX_POINTS)
            K = self._closest_k[key]
        else:
            K = int(max_points)
            if K < 0:
                raise ValueError('max_points must be >= 0, got %d' % K)
        B = self.num_envs
        need_ids = 'id' in want and K > 0
        need_geom = K > 0 and any(g in want for g in ('pos', 'normal', 'distance'))
        if K > 0 and not (need_ids or need_geom):
            raise ValueError("max_points %d with none of 'id', 'pos', 'normal', 'distance' wanted: nowhere to put the rows" % K)
        near = 'nearest' in want
        key = (need_ids, need_geom, near, K)
        if key not in self._closest_out:
            Ks = max(K, 1)   # (K = 0: the buffers still exist, the views are empty)
            dev = self.device
            self._closest_out[key] = (torch.zeros((B, ), dtype=torch.int32, device=dev),
                                      torch.empty((B, Ks, 2), dtype=torch.int32, device=dev) if need_ids else None,
                                      torch.empty((B, Ks, 10), dtype=torch.float32, device=dev) if need_geom else None,
                                      torch.empty((B, 2), dtype=torch.int32, device=dev) if near else None,
                                      torch.empty((B, 10), dtype=torch.float32, device=dev) if near else None)
        if self._closest_scratch is None:
            self._closest_scratch = torch.empty((max(int(self.lib.dg_world_closest_scratch_floats(self.handle)), 1), ), dtype=torch.float32,
                                                device=self.device)
        count, ids, geom, nids, ngeom = self._closest_out[key]
        self._dyn_check(self.lib.dg_world_closest(self.handle, _ptr(self.state), ba, la, bb, lb, distance, K, _ptr(self._closest_scratch), _ptr(count),
                                                  _ptr(ids), _ptr(geom), _ptr(nids), _ptr(ngeom), self._stream()))
        pos, nrm, dist = K > 0 and 'pos' in want, K > 0 and 'normal' in want, K > 0 and 'distance' in want
        empty = lambda *s: torch.empty((B, 0) + s, dtype=torch.float32, device=self.device)
        return ClosestPoints(
            count,
            (ids[:, :K, 0] if K > 0 else torch.empty((B, 0), dtype=torch.int32, device=self.device)) if 'id' in want else None,
            (ids[:, :K, 1] if K > 0 else torch.empty((B, 0), dtype=torch.int32, device=self.device)) if 'id' in want else None,
            (geom[:, :K, 0:3] if pos else empty(3)) if 'pos' in want else None, (geom[:, :K, 3:6] if pos else empty(3)) if 'pos' in want else None,
            (geom[:, :K, 6:9] if nrm else empty(3)) if 'normal' in want else None, (geom[:, :K, 9] if dist else empty()) if 'distance' in want else None,
            nids[:, 0] if near else None, nids[:, 1] if near else None, ngeom[:, 0:3] if near else None, ngeom[:, 3:6] if near else None,
            ngeom[:, 6:9] if near else None, ngeom[:, 9] if near else None)

    def set_render_diag(self, flags):
        """Diagnostic switches of ``render`` (1: no culling -- the brute-force picture; see dg_world_set_render_diag)."""
        self._check(self.lib.dg_world_set_render_diag(self.handle, int(flags)))

    def motor_cfg(self):
        cfg = np.zeros((self.n_links, 3), dtype=np.float64)
        self._check(self.lib.dg_world_get_motor_cfg(self.handle, cfg.ctypes.data_as(_c_f64p)))
        return cfg

    def set_motor_cfg(self, cfg):
        cfg = np.ascontiguousarray(cfg, dtype=np.float64)
        self._check(self.lib.dg_world_set_motor_cfg(self.handle, cfg.ctypes.data_as(_c_f64p)))

    # columns of the diagnostics buffer (include/diygym_hip.h DG_DIAG_*)
    DIAG_STRIDE, DIAG_CONTACTS, DIAG_PGS_ITERS, DIAG_PGS_ITERS_FIRST, DIAG_CONTACTS_FIRST, DIAG_IK_ITERS, DIAG_N_IK = 8, 0, 1, 2, 3, 4, 4

    def enable_diagnostics(self):
        self.diag = torch.zeros((self.num_envs, self.DIAG_STRIDE), dtype=torch.int32, device=self.device)
        self._check(self.lib.dg_world_set_diag_buffer(self.handle, _ptr(self.diag)))
        return self.diag

    def disable_diagnostics(self):
        self._check(self.lib.dg_world_set_diag_buffer(self.handle, None))

    def enable_skip_counter(self):
        """int32 [num_envs]: with every step, how many of its substeps ran without narrow phase and pose pass (the clearance
        measured by the previous narrow phase exceeded what the arms could have moved; dg_world_set_skip_counter)."""
        self.skipped = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self._check(self.lib.dg_world_set_skip_counter(self.handle, _ptr(self.skipped)))
        return self.skipped

    def disable_skip_counter(self):
        self._check(self.lib.dg_world_set_skip_counter(self.handle, None))

    @property
    def kernel_name(self):
        return self.lib.dg_world_kernel_name(self.handle).decode()

    @property
    def par(self):
        """True when the step runs as the four-wavefront helper-wave kernel."""
        return self.kernel_name.startswith('step_kernel_par')

    SECTIONS = ['update_ops', 'kinematics', 'narrow_phase', 'aba', 'minv', 'rows', 'pgs_other', 'integrate', 'outputs', 'pgs_motor', 'pgs_limit',
                'pgs_contact']

    @property
    def envs_per_wave(self):
        """Envs per wavefront of the workspace mode (``lanes``: 64/32/16/8/4/1 LDS modes, 0 and -16 global-workspace modes).

        The mode is chosen per scene AND batch size (and, for one-env-per-wavefront scenes, the GPU's CU count): each
        mode sums in its own order, so a rollout replays bit for bit only within one mode.  Shards of a job that must
        equal the whole batch bit for bit pin the mode with the environment variable ``DG_MAX_LANES`` (32 / 16 / 8 / 4 /
        1) before constructing their worlds; ``sim.lanes`` tells which mode a world got."""
        return self.lanes if self.lanes > 0 else (-self.lanes if self.lanes < 0 else 64)

    def enable_stamps(self, on=True):
        """Diagnostic: per-wavefront shader cycles per section of the step (see diygym_hip.h)."""
        if on:
            n_waves = (self.num_envs + self.envs_per_wave - 1) // self.envs_per_wave
            self.cycles = torch.zeros((n_waves, len(self.SECTIONS) + 12), dtype=torch.int64, device=self.device)
            self._check(self.lib.dg_world_set_profile_buffer(self.handle, _ptr(self.cycles)))
        else:
            self._check(self.lib.dg_world_set_profile_buffer(self.handle, None))
        return getattr(self, 'cycles', None)

    # state as [num_envs, state_dim] host array (tests / checkpoints)
    def get_state(self):
        return self.state[:, :self.num_envs].t().contiguous().cpu().numpy()

    def set_state(self, arr):
        t = torch.as_tensor(np.asarray(arr, dtype=np.float32), device=self.device)
        if tuple(t.shape) != (self.num_envs, self.state_dim):
            raise ValueError('state must have shape %s, got %s' % ((self.num_envs, self.state_dim), tuple(t.shape)))
        self.state[:, :self.num_envs] = t.t()

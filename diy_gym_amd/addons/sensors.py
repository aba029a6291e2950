"""Sensor addons, compiled to observe-phase ops of the batched step kernel."""
from collections import OrderedDict

import numpy as np

from .. import spaces
from ..scene import K
from .addon import Addon


class JointStateSensor(Addon):
    """Joint position (+ velocity, default ON; + effort) (reference:
    diy_gym/addons/sensors/joint_state_sensor.py:15-57).  Effort is the motor
    torque applied during the last solver pass (``getJointStates`` item 3)."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        self.uid = parent.uid
        robot = parent.robot
        if 'joints' in config:
            names = robot.joint_names
            self.joint_ids = [names.index(j) for j in config.get('joints')]
        else:
            self.joint_ids = [j.index for j in robot.joints if j.q_index > -1]
        for j in self.joint_ids:
            if robot.joints[j].q_index < 0:
                raise ValueError('joint_state_sensor: joint %s is fixed and has no state' % robot.joints[j].name)
        self.include_velocity = config.get('include_velocity', True)
        self.include_effort = config.get('include_effort', False)
        info = [robot.joints[j] for j in self.joint_ids]
        sp = OrderedDict(position=spaces.Box(low=np.array([j.lower for j in info]), high=np.array([j.upper for j in info]),
                                             dtype='float32'))
        if self.include_velocity:
            vmax = np.array([j.velocity for j in info])
            sp['velocity'] = spaces.Box(low=-vmax, high=vmax, dtype='float32')
        if self.include_effort:
            tmax = np.array([j.effort for j in info])
            sp['effort'] = spaces.Box(low=-tmax, high=tmax, dtype='float32')
        self.observation_space = spaces.Dict(sp)

    def compile(self, builder):
        dofs = [builder.global_link(self.uid, self.parent.robot.joints[j].q_index) for j in self.joint_ids]
        n = len(dofs)
        flags = (K.JS_VELOCITY if self.include_velocity else 0) | (K.JS_EFFORT if self.include_effort else 0)
        self.op = builder.add_op(K.OP_OBS_JOINT_STATE, 'obs', body=self.uid, flags=flags, ilist=dofs,
                                 io_dim=n * (1 + bool(self.include_velocity) + bool(self.include_effort)))
        self._n = n

    def observe(self):
        env, off, n = self.env, self.op.io_off, self._n
        obs = OrderedDict(position=env._obs_view(off, n))
        k = off + n
        if self.include_velocity:
            obs['velocity'] = env._obs_view(k, n)
            k += n
        if self.include_effort:
            obs['effort'] = env._obs_view(k, n)
        return obs


class ObjectStateSensor(Addon):
    """Pose / twist of a model's base or link, optionally minus a source frame's
    (reference: diy_gym/addons/sensors/object_state_sensor.py:8-83).  Kept quirks:
    the link path reads the *inertial* frame (items 0,1,6,7); with a source the
    subtraction is done in the world frame and ``rotation`` is
    ``q_source (x) q_target``, not a relative rotation; ``angular_velocity`` needs
    both ``include_rotation`` and ``include_velocity``."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        self.source_model = parent.models[config.get('source_model')] if 'source_model' in config else None
        self.target_model = parent.models[config.get('target_model')] if 'target_model' in config else parent
        self.source_frame_id = self.source_model.get_frame_id(config.get('source_frame')) if 'source_frame' in config else -1
        self.target_frame_id = self.target_model.get_frame_id(config.get('target_frame')) if 'target_frame' in config else -1
        self.include_rotation = config.get('include_rotation', False)
        self.include_velocity = config.get('include_velocity', False)
        box = lambda: spaces.Box(-10, 10, shape=(3, ), dtype='float32')
        sp = OrderedDict(position=box())
        if self.include_rotation:
            sp['rotation'] = box()
        if self.include_velocity:
            sp['velocity'] = box()
        if self.include_rotation and self.include_velocity:
            sp['angular_velocity'] = box()
        self.observation_space = spaces.Dict(sp)

    def compile(self, builder):
        flags = (K.OS_ROTATION if self.include_rotation else 0) | (K.OS_VELOCITY if self.include_velocity else 0)
        n = 3 * (1 + bool(self.include_rotation) + bool(self.include_velocity) +
                 bool(self.include_rotation and self.include_velocity))
        src = self.source_model
        self.op = builder.add_op(K.OP_OBS_OBJECT_STATE, 'obs', body=self.target_model.uid, frame=self.target_frame_id,
                                 body2=src.uid if src is not None else -1, frame2=self.source_frame_id, flags=flags,
                                 io_dim=n)

    def observe(self):
        # dict order as built by the reference's observe(): position, velocity, rotation, angular_velocity
        env, k = self.env, self.op.io_off
        obs = OrderedDict(position=env._obs_view(k, 3))
        k += 3
        if self.include_velocity:
            obs['velocity'] = env._obs_view(k, 3)
            k += 3
        if self.include_rotation:
            obs['rotation'] = env._obs_view(k, 3)
            k += 3
        if self.include_rotation and self.include_velocity:
            obs['angular_velocity'] = env._obs_view(k, 3)
        return obs


class ForceTorqueSensor(Addon):
    """Reaction wrench across one joint of the parent model: ``force`` and ``torque`` (reference:
    diy_gym/addons/sensors/force_torque_sensor.py:8-23 -- ``enableJointForceTorqueSensor`` + ``getJointState()[2]``).

    What is reported [R: Bullet's joint feedback, ``I^A a + Z^A`` of the child link in its own frame]: the force and
    the torque the PARENT side exerts on the CHILD side through the joint -- gravity, inertial loads and the contact
    forces acting on the child side all show -- expressed in the child link's inertial frame, torque about its
    origin.  Computed in the output phase by Newton-Euler over the child side (the rigid cluster of URDF links behind
    the joint plus every moving link hanging off it), with the accelerations of the step's LAST substep,
    ``(v_end - v_start) / h``, and that substep's contact impulses.  ``frame`` names the joint (fixed or movable); it
    is required: the reference's default of -1 makes ``getJointState`` fail."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        if 'frame' not in config:
            raise ValueError("force_torque_sensor needs a 'frame' (the reference's default, joint -1, is rejected by pybullet)")
        self.uid = parent.uid
        self.frame_id = parent.get_frame_id(config.get('frame'))
        if self.frame_id < 0:
            raise ValueError('force_torque_sensor: model %r has no joint %r' % (parent.name, config.get('frame')))
        box = lambda: spaces.Box(-10, 10, shape=(3, ), dtype='float32')
        self.observation_space = spaces.Dict(OrderedDict(force=box(), torque=box()))

    def compile(self, builder):
        if self.uid in builder.aliases:
            raise NotImplementedError('force_torque_sensor on an attached child model')
        flat = self.parent.flat
        cl = flat.ft_cluster(self.frame_id)
        m, c, I = cl['rigid']
        whole = self.parent.robot.joints[self.frame_id].movable
        shapes = builder.shapes_of(self.uid, cl['urdf_links'], cl['moving'])
        moving = [builder.global_link(self.uid, d) for d in cl['moving']]
        self.op = builder.add_op(K.OP_OBS_FT, 'obs', body=self.uid, frame=self.frame_id, flags=K.FT_WHOLE_LINK if whole else 0,
                                 ilist=[len(moving)] + moving + [len(shapes)] + shapes,
                                 flist=[m, c[0], c[1], c[2], I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]], io_dim=6,
                                 state_dim=builder.prev_velocity_slots(self.uid))

    def observe(self):
        off = self.op.io_off
        return OrderedDict(force=self.env._obs_view(off, 3), torque=self.env._obs_view(off + 3, 3))


class Camera(Addon):
    """RGB (+ depth, default ON; + segmentation) from a pinhole camera attached to a model frame or fixed in
    the world (reference: diy_gym/addons/sensors/camera.py:26-98).  Same config keys and defaults
    (``clipping_boundaries`` [0.01, 100], ``field_of_view`` 70, ``resolution`` [640, 480], ``frame``, ``xyz``,
    ``rpy``, ``use_depth`` True, ``use_segmentation_mask`` False).  Rendered by its own kernel launch
    (``dg_world_render``), lazily, the first time ``observe()`` is called after a step.

    * ``depth`` is what the reference's formula (:82-85) yields: the eye-space z of the nearest surface,
      i.e. NEGATIVE values in [-far, -near]; -far where the ray hits nothing.
    * ``segmentation_mask`` is ``uid + ((link + 1) << 24)``, -1 for background.
    * ``rgb`` is flat-shaded collision geometry -- not comparable with pybullet's lit visual meshes.
    * Images are the row-major ``height x width`` buffer viewed with shape ``resolution`` (= [w, h]),
      exactly like the reference's ``reshape`` (:77), so non-square images are scrambled there too.
    """
    def __init__(self, parent, config):
        super().__init__(parent, config)
        from ..mathx import Transform, quat_from_euler
        from ..model import Model
        self.near, self.far = config.get('clipping_boundaries', [0.01, 100])
        self.fov = config.get('field_of_view', 70.0)
        self.resolution = list(config.get('resolution', [640, 480]))
        self.aspect = self.resolution[0] / self.resolution[1]
        self.uid = parent.uid if isinstance(parent, Model) else -1
        self.frame_id = parent.get_frame_id(config.get('frame')) if 'frame' in config else -1
        xyz = config.get('xyz', [0., 0., 0.])
        rpy = config.get('rpy', [0., 0., 0.])
        self.use_depth = config.get('use_depth', True)
        self.use_seg_mask = config.get('use_segmentation_mask', False)
        self.T_parent_cam = Transform.from_xyz_quat(xyz, quat_from_euler(rpy))
        sp = OrderedDict(rgb=spaces.Box(0., 1., shape=self.resolution + [3], dtype='float32'))
        if self.use_depth:
            sp['depth'] = spaces.Box(0., 10., shape=self.resolution, dtype='float32')
        if self.use_seg_mask:
            sp['segmentation_mask'] = spaces.Box(0., 10., shape=self.resolution, dtype='float32')
        self.observation_space = spaces.Dict(sp)
        self._tick = None
        self._buffers = None

    def compile(self, builder):
        from ..scene import K as _K
        flags = (_K.CAM_DEPTH if self.use_depth else 0) | (_K.CAM_SEGMENTATION if self.use_seg_mask else 0)
        self.camera_index = builder.add_camera(self.uid, self.frame_id, self.resolution[0], self.resolution[1], flags,
                                               self.T_parent_cam, self.fov, self.near, self.far)

    def observe(self):
        import torch
        env = self.env
        B, (w, h) = env.num_envs, self.resolution
        if self._buffers is None:
            dev = env.device
            self._buffers = (torch.zeros((B, w, h, 3), dtype=torch.float32, device=dev),
                             torch.zeros((B, w, h), dtype=torch.float32, device=dev) if self.use_depth else None,
                             torch.zeros((B, w, h), dtype=torch.int32, device=dev) if self.use_seg_mask else None)
        rgb, depth, seg = self._buffers
        if self._tick != env._tick:
            env.sim.render(self.camera_index, rgb, depth, seg)
            self._tick = env._tick
        obs = OrderedDict(rgb=env._out(rgb))
        if self.use_depth:
            obs['depth'] = env._out(depth)
        if self.use_seg_mask:
            obs['segmentation_mask'] = env._out(seg)
        return obs


class Lidar(Addon):
    """Range scan by batched ray casting against the collision geometry (``env.sim.ray_test_batch`` -- pybullet's
    ``p.rayTestBatch``; the reference ships no such addon).  Attaches to a model frame or to the world exactly like
    ``camera`` (``frame``, ``xyz``, ``rpy``).  Sensor frame: x forward, z up; azimuth turns about z, elevation tilts
    towards z.  Config keys: ``num_rays`` 64 (per ring), ``num_rings`` 1, ``horizontal_fov`` [-180, 180] degrees (the end
    is left out when the fan spans 360 degrees: no doubled ray), ``vertical_fov`` [0, 0] degrees (the rings' elevations),
    ``range`` [0.05, 10.0] (rays run from ``min`` to ``max`` along each direction), ``ignore_parent`` True (no ray can hit
    the model the sensor sits on), ``use_ids`` False.

    * ``ranges`` ``[num_rings, num_rays]``: metres from the sensor origin to the nearest surface, ``max`` where nothing is hit.
    * ``ids`` (with ``use_ids``) int32, same shape: ``uid + ((link + 1) << 24)`` as the camera's segmentation mask, -1 = nothing.

    Evaluated by its own two kernel launches (``dg_world_raycast``), lazily, the first time ``observe()`` is called after a step."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        from ..mathx import Transform, quat_from_euler
        from ..model import Model
        self.num_rays = int(config.get('num_rays', 64))
        self.num_rings = int(config.get('num_rings', 1))
        self.horizontal_fov = [float(v) for v in config.get('horizontal_fov', [-180., 180.])]
        self.vertical_fov = [float(v) for v in config.get('vertical_fov', [0., 0.])]
        self.range_min, self.range_max = (float(v) for v in config.get('range', [0.05, 10.0]))
        if self.num_rays < 1 or self.num_rings < 1 or not 0.0 <= self.range_min < self.range_max:
            raise ValueError('lidar: num_rays and num_rings must be >= 1 and range [min, max] must satisfy 0 <= min < max')
        self.uid = parent.uid if isinstance(parent, Model) else -1
        self.frame_id = parent.get_frame_id(config.get('frame')) if 'frame' in config else -1
        self.ignore_parent = bool(config.get('ignore_parent', True))
        self.use_ids = bool(config.get('use_ids', False))
        T = Transform.from_xyz_quat(config.get('xyz', [0., 0., 0.]), quat_from_euler(config.get('rpy', [0., 0., 0.])))
        self.T_parent_sensor = T
        # ray directions, built once: [num_rings * num_rays, 3] in the sensor frame, then the segments in the parent frame
        lo, hi = self.horizontal_fov
        n = self.num_rays
        if abs(hi - lo) >= 360.0 - 1e-9:
            az = lo + (hi - lo) * np.arange(n) / n
        else:
            az = np.linspace(lo, hi, n)
        el = np.linspace(self.vertical_fov[0], self.vertical_fov[1], self.num_rings)
        az, el = np.radians(az)[None, :], np.radians(el)[:, None]
        dirs = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1).reshape(-1, 3)
        self.directions = dirs
        self.ray_from = (T.p[None, :] + (dirs * self.range_min) @ T.R.T).astype(np.float32)
        self.ray_to = (T.p[None, :] + (dirs * self.range_max) @ T.R.T).astype(np.float32)
        shape = [self.num_rings, self.num_rays]
        sp = OrderedDict(ranges=spaces.Box(0., self.range_max, shape=shape, dtype='float32'))
        if self.use_ids:
            sp['ids'] = spaces.Box(-1, np.iinfo(np.int32).max, shape=shape, dtype='int32')
        self.observation_space = spaces.Dict(sp)
        self.own_buffers = True   # like a camera's pictures, the scan is not part of the kernel's observation rows
        self._tick = None
        self._rays = None

    def compile(self, builder):
        pass   # rays are run-time arguments of dg_world_raycast: nothing in the scene blob

    def observe(self):
        import torch
        env = self.env
        if self._rays is None:
            self._rays = (torch.as_tensor(self.ray_from, device=env.device).contiguous(), torch.as_tensor(self.ray_to, device=env.device).contiguous())
        if self._tick != env._tick:
            hits = env.sim.ray_test_batch(self._rays[0], self._rays[1], body=self.uid, frame=self.frame_id,
                                          skip_body=self.uid if self.ignore_parent else -1, want=('frac', 'id') if self.use_ids else ('frac', ))
            shape = (env.num_envs, self.num_rings, self.num_rays)
            self._ranges = (self.range_min * (1.0 - hits.frac) + self.range_max * hits.frac).reshape(shape)   # (frac = 1, a miss: max exactly)
            self._ids = hits.id.reshape(shape).clone() if self.use_ids else None   # (the backend reuses its output tensors)
            self._tick = env._tick
        obs = OrderedDict(ranges=env._out(self._ranges))
        if self.use_ids:
            obs['ids'] = env._out(self._ids)
        return obs


class ContactSensor(Addon):
    """Touch and normal force on a model by the batched contact query (``env.sim.contact_points`` -- pybullet's
    ``p.getContactPoints``; the reference ships no such addon).  Goes on a model.  Config keys: ``target`` (the name of another
    model of the scene; default: contacts with any body), ``frame`` (a joint of the parent: only that link's contacts; default:
    every link of the parent), ``terminal`` False, ``force_threshold`` 0.0 N (used with ``terminal``).

    * ``touching`` ``[1]``: 1.0 when at least one matching contact has ``distance <= 0`` (the narrow phase also lists contacts
      that are up to ``contact_margin`` apart: those do not count).
    * ``force`` ``[1]``: the sum of the matching contacts' normal forces in newtons -- what the solver applied in the last
      substep (``dg_world_contacts`` has the staleness rule); it needs the scene's contact impulse cache (``warmstart`` > 0).
    * ``is_terminal()`` with ``terminal``: ``touching`` and ``force >= force_threshold``.

    Evaluated by its own kernel launch (``dg_world_contacts``), lazily, the first time ``observe()`` or ``is_terminal()`` is called
    after a step."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        from ..model import Model
        if not isinstance(parent, Model):
            raise ValueError('contact_sensor goes on a model, not on the environment')
        self.uid = parent.uid
        self.target_name = config.get('target') if 'target' in config else None
        self.frame_id = None
        if 'frame' in config:
            self.frame_id = parent.get_frame_id(config.get('frame'))
            if self.frame_id < 0:
                raise ValueError('contact_sensor: model %r has no joint %r' % (parent.name, config.get('frame')))
        self.terminal = bool(config.get('terminal', False))
        self.force_threshold = float(config.get('force_threshold', 0.0))
        box = lambda hi: spaces.Box(0., hi, shape=(1, ), dtype='float32')
        self.observation_space = spaces.Dict(OrderedDict(touching=box(1.), force=box(np.inf)))
        self.own_buffers = True   # like a lidar's scan, not part of the kernel's observation rows
        self.late_terminal = self.terminal   # its terminal is evaluated after the step kernel: the env folds it into the collapsed flag
        self.target_uid = None
        self._tick = None

    def compile(self, builder):
        # (nothing in the scene blob: the filters are run-time arguments of dg_world_contacts; every model exists by now)
        if self.target_name is not None:
            models = self.env.models
            if self.target_name not in models:
                raise ValueError('contact_sensor: the scene has no model %r' % (self.target_name, ))
            self.target_uid = models[self.target_name].uid

    def _evaluate(self):
        import torch
        env = self.env
        if self._tick != env._tick:
            if not hasattr(env.sim, 'contact_points'):
                raise NotImplementedError('contact_sensor needs a backend with the batched contact query (contact_points); %s has none'
                                          % type(env.sim).__name__)
            cp = env.sim.contact_points(self.uid, self.target_uid, self.frame_id, None, want=('distance', 'force'))
            C = cp.distance.shape[1]
            live = torch.arange(C, device=env.device, dtype=torch.int32)[None, :] < cp.count[:, None]
            self._touching = (live & (cp.distance <= 0.0)).any(dim=1, keepdim=True)
            self._force = cp.normal_force.sum(dim=1, keepdim=True)   # (the slots behind the count are 0: no mask)
            self._tick = env._tick

    def observe(self):
        self._evaluate()
        return OrderedDict(touching=self.env._out(self._touching.float()), force=self.env._out(self._force))

    def is_terminal(self):
        if not self.terminal:
            return None
        self._evaluate()
        return self.env._out((self._touching & (self._force >= self.force_threshold))[:, 0])


class ContactForceSensor(Addon):
    """Net contact force (and moment) on links of a model by the batched net contact wrench (``env.sim.net_contact_forces`` --
    normal AND friction forces, what ``contact_sensor`` leaves out; the reference ships no such addon, its ``force_torque_sensor``
    reads a joint's wrench, not a surface's).  Goes on a model.  Config keys: ``frames`` (a list of joints of the parent: one row
    per link; default: one row for the whole body), ``target`` (the name of another model of the scene; default: contacts with
    any body), ``use_torque`` False (needs ``frames``: a moment needs a link to be taken about).

    * ``force`` ``[3 n]``: per row the sum of the forces its contacts apply to the parent, world axes, newtons -- a foot's ground
      reaction, a finger's grip and traction.
    * ``torque`` ``[3 n]`` (with ``use_torque``): the sum of their moments about the origin of the link's inertial frame.

    What the solver applied in the last substep (``dg_world_net_contact_wrench`` has the staleness rule); it needs the scene's
    contact impulse cache (``warmstart`` > 0).  Evaluated by ONE kernel launch of its own, lazily, the first time ``observe()`` is
    called after a step."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        from ..model import Model
        if not isinstance(parent, Model):
            raise ValueError('contact_force_sensor goes on a model, not on the environment')
        self.uid = parent.uid
        self.target_name = config.get('target') if 'target' in config else None
        self.frame_ids = None
        if 'frames' in config:
            names = config.get('frames')
            names = [names] if isinstance(names, str) else list(names)
            if not 1 <= len(names) <= 16:
                raise ValueError('contact_force_sensor: frames takes 1 .. 16 joints, got %d' % len(names))
            self.frame_ids = [parent.get_frame_id(n) for n in names]
            for n, f in zip(names, self.frame_ids):
                if f < 0:
                    raise ValueError('contact_force_sensor: model %r has no joint %r' % (parent.name, n))
        self.use_torque = bool(config.get('use_torque', False))
        if self.use_torque and self.frame_ids is None:
            raise ValueError('contact_force_sensor: use_torque needs frames (the links the moments are taken about)')
        n = 1 if self.frame_ids is None else len(self.frame_ids)
        box = lambda: spaces.Box(-np.inf, np.inf, shape=(3 * n, ), dtype='float32')
        self.observation_space = spaces.Dict(OrderedDict([('force', box())] + ([('torque', box())] if self.use_torque else [])))
        self.own_buffers = True   # like contact_sensor's, not part of the kernel's observation rows
        self.target_uid = None
        self._tick = None

    def compile(self, builder):
        # (nothing in the scene blob: body, links and filter are run-time arguments of dg_world_net_contact_wrench)
        if self.target_name is not None:
            models = self.env.models
            if self.target_name not in models:
                raise ValueError('contact_force_sensor: the scene has no model %r' % (self.target_name, ))
            self.target_uid = models[self.target_name].uid

    def observe(self):
        env = self.env
        if self._tick != env._tick:
            if not hasattr(env.sim, 'net_contact_forces'):
                raise NotImplementedError('contact_force_sensor needs a backend with the batched net contact wrench (net_contact_forces); %s has none'
                                          % type(env.sim).__name__)
            force, torque, _ = env.sim.net_contact_forces(self.uid, self.frame_ids, self.target_uid, None,
                                                          want=('force', 'torque') if self.use_torque else ('force', ))
            B = force.shape[0]
            self._force = force.reshape(B, -1).clone()   # (the backend reuses its output tensors)
            self._torque = torque.reshape(B, -1).clone() if self.use_torque else None
            self._tick = env._tick
        obs = OrderedDict(force=env._out(self._force))
        if self.use_torque:
            obs['torque'] = env._out(self._torque)
        return obs


class ProximitySensor(Addon):
    """Clearance of a model from the bodies around it by the batched closest-points query (``env.sim.closest_points`` --
    pybullet's ``p.getClosestPoints``; the reference ships no such addon).  Goes on a model.  Config keys: ``target`` (the name of
    another model of the scene; default: any other body), ``frame`` (a joint of the parent: only that link's shapes; default: every
    link of the parent), ``range`` 0.5 m, ``terminal`` False, ``threshold`` 0.0 m (used with ``terminal``).

    * ``distance`` ``[1]``: the smallest distance between a shape of the parent and a shape of the target, negative when they
      overlap; ``range`` when nothing is nearer than that.
    * ``direction`` ``[3]``: the unit vector from the parent towards the nearest body (minus the query's normal); 0 when nothing
      is within ``range``.
    * ``is_terminal()`` with ``terminal``: ``distance < threshold``.

    Evaluated by its own two launches (``dg_world_closest`` with ``max_points=0``: the nearest pair alone), lazily, the first time
    ``observe()`` or ``is_terminal()`` is called after a step."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        from ..model import Model
        if not isinstance(parent, Model):
            raise ValueError('proximity_sensor goes on a model, not on the environment')
        self.uid = parent.uid
        self.target_name = config.get('target') if 'target' in config else None
        self.frame_id = None
        if 'frame' in config:
            self.frame_id = parent.get_frame_id(config.get('frame'))
            if self.frame_id < 0:
                raise ValueError('proximity_sensor: model %r has no joint %r' % (parent.name, config.get('frame')))
        self.range = float(config.get('range', 0.5))
        if not (np.isfinite(self.range) and self.range >= 0.0):
            raise ValueError('proximity_sensor: range must be finite and >= 0, got %r' % (self.range, ))
        self.terminal = bool(config.get('terminal', False))
        self.threshold = float(config.get('threshold', 0.0))
        self.observation_space = spaces.Dict(OrderedDict(distance=spaces.Box(-np.inf, self.range, shape=(1, ), dtype='float32'),
                                                         direction=spaces.Box(-1., 1., shape=(3, ), dtype='float32')))
        self.own_buffers = True   # like a lidar's scan, not part of the kernel's observation rows
        self.late_terminal = self.terminal   # evaluated after the step kernel: the env folds it into the collapsed flag
        self.target_uid = None
        self._tick = None

    def compile(self, builder):
        # (nothing in the scene blob: the filters are run-time arguments of dg_world_closest; every model exists by now)
        if self.target_name is not None:
            models = self.env.models
            if self.target_name not in models:
                raise ValueError('proximity_sensor: the scene has no model %r' % (self.target_name, ))
            self.target_uid = models[self.target_name].uid

    def _evaluate(self):
        env = self.env
        if self._tick != env._tick:
            if not hasattr(env.sim, 'closest_points'):
                raise NotImplementedError('proximity_sensor needs a backend with the batched closest-points query (closest_points); %s has none'
                                          % type(env.sim).__name__)
            cp = env.sim.closest_points(self.uid, self.target_uid, self.range, self.frame_id, None, max_points=0, want=('nearest', ))
            self._distance = cp.nearest_distance.reshape(-1, 1).clone()   # (the backend reuses its output tensors)
            self._direction = -cp.nearest_normal
            self._tick = env._tick

    def observe(self):
        self._evaluate()
        return OrderedDict(distance=self.env._out(self._distance), direction=self.env._out(self._direction))

    def is_terminal(self):
        if not self.terminal:
            return None
        self._evaluate()
        return self.env._out(self._distance[:, 0] < self.threshold)


class LinkStateSensor(Addon):
    """Poses -- and on request velocities -- of several links of a model by the batched link-state query (``env.sim.link_states``
    -- pybullet's ``p.getLinkStates``; the reference ships no such addon, its ``object_state_sensor`` reads one frame).  A keypoint
    observation in ONE launch per step.  Goes on a model.  Config keys: ``frames`` (a list of joints of the parent, ``base`` for
    the base link; default: the base alone), ``com`` False (the links' INERTIAL frames instead of their URDF frames),
    ``use_velocity`` False.

    Observations are in world coordinates, one row per frame in ``frames`` order:

    * ``position`` ``[3 n]``, ``orientation`` ``[4 n]`` (quaternion xyzw);
    * with ``use_velocity``, ``velocity`` ``[3 n]`` and ``angular_velocity`` ``[3 n]``.

    Evaluated by its own kernel launch (``dg_world_link_states``), lazily, the first time ``observe()`` is called after a step."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        from ..model import Model
        if not isinstance(parent, Model):
            raise ValueError('link_state_sensor goes on a model, not on the environment')
        self.uid = parent.uid
        names = config.get('frames') if 'frames' in config else ['base']
        names = [names] if isinstance(names, str) else list(names)
        if not 1 <= len(names) <= 32:
            raise ValueError('link_state_sensor: frames takes 1 .. 32 joints, got %d' % len(names))
        self.frame_ids = [parent.get_frame_id(n) for n in names]   # (-1, the base, for a name that is no joint: only `base` may be)
        for n, f in zip(names, self.frame_ids):
            if f < 0 and n != 'base':
                raise ValueError('link_state_sensor: model %r has no joint %r' % (parent.name, n))
        self.com = bool(config.get('com', False))
        self.use_velocity = bool(config.get('use_velocity', False))
        n = len(names)
        box = lambda k, hi=np.inf: spaces.Box(-hi, hi, shape=(k * n, ), dtype='float32')
        sp = OrderedDict(position=box(3), orientation=box(4, 1.))
        if self.use_velocity:
            sp['velocity'], sp['angular_velocity'] = box(3), box(3)
        self.observation_space = spaces.Dict(sp)
        self.own_buffers = True   # like contact_sensor's, not part of the kernel's observation rows
        self._tick = None

    def compile(self, builder):
        pass   # nothing in the scene blob: the selectors are run-time arguments of dg_world_link_states

    def observe(self):
        env = self.env
        if self._tick != env._tick:
            if not hasattr(env.sim, 'link_states'):
                raise NotImplementedError('link_state_sensor needs a backend with the batched link-state query (link_states); %s has none'
                                          % type(env.sim).__name__)
            st = env.sim.link_states(self.uid, self.frame_ids, com=self.com)
            B = st.shape[0]
            cols = lambda a, b: st[:, :, a:b].reshape(B, -1).contiguous()   # (a copy, also for n = 1: the backend reuses its output tensor)
            self._obs = OrderedDict(position=cols(0, 3), orientation=cols(3, 7))
            if self.use_velocity:
                self._obs['velocity'], self._obs['angular_velocity'] = cols(7, 10), cols(10, 13)
            self._tick = env._tick
        return OrderedDict((k, env._out(v)) for k, v in self._obs.items())


class JointWrenchSensor(Addon):
    """Reaction wrenches across several joints of a model -- and on request the motors' applied torques -- by the batched joint
    reaction query (``env.sim.joint_reaction_forces`` / ``joint_motor_torques``: the second half of pybullet's ``p.getJointStates``;
    the reference's ``force_torque_sensor`` reads one joint).  A wrist wrench, torque residuals for collision detection or a load
    penalty over all joints in ONE launch per step.  Goes on a model.  Config keys: ``frames`` (a list of 1 .. 16 joints of the
    parent, fixed or movable; default: every movable joint), ``use_motor_torque`` False.

    * ``force`` ``[3 n]``, ``torque`` ``[3 n]``: per joint, in ``frames`` order, what the compiled ``force_torque_sensor`` reports --
      the force and torque the parent side exerts on the child side, in the inertial frame of the joint's child link, torque about
      its origin (``env.sim.joint_reaction_forces`` has the semantics and the staleness rule in full).
    * ``motor_torque`` ``[nv]`` (with ``use_motor_torque``): the torque each motor applied in the last solver pass.

    ``compile()`` makes the scene keep the model's velocities at the start of the last substep
    (``builder.enable_joint_force_torque``).  Evaluated by ONE kernel launch of its own (two with ``use_motor_torque``), lazily, the
    first time ``observe()`` is called after a step."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        from ..model import Model
        if not isinstance(parent, Model):
            raise ValueError('joint_wrench_sensor goes on a model, not on the environment')
        self.uid = parent.uid
        robot = parent.robot
        if 'frames' in config:
            names = config.get('frames')
            names = [names] if isinstance(names, str) else list(names)
            self.frame_ids = [parent.get_frame_id(n) for n in names]
            for n, f in zip(names, self.frame_ids):
                if f < 0:
                    raise ValueError('joint_wrench_sensor: model %r has no joint %r' % (parent.name, n))
        else:
            self.frame_ids = [j.index for j in robot.joints if j.q_index > -1]
        if not 1 <= len(self.frame_ids) <= 16:
            raise ValueError('joint_wrench_sensor: frames takes 1 .. 16 joints, got %d' % len(self.frame_ids))
        self.use_motor_torque = bool(config.get('use_motor_torque', False))
        n = len(self.frame_ids)
        box = lambda k: spaces.Box(-np.inf, np.inf, shape=(k, ), dtype='float32')
        sp = OrderedDict(force=box(3 * n), torque=box(3 * n))
        if self.use_motor_torque:
            sp['motor_torque'] = box(sum(1 for j in robot.joints if j.q_index > -1))
        self.observation_space = spaces.Dict(sp)
        self.own_buffers = True   # like contact_force_sensor's, not part of the kernel's observation rows
        self._tick = None

    def compile(self, builder):
        builder.enable_joint_force_torque(self.uid)   # (the selectors are run-time arguments of dg_world_joint_wrench)

    def observe(self):
        env = self.env
        if self._tick != env._tick:
            if not hasattr(env.sim, 'joint_reaction_forces'):
                raise NotImplementedError('joint_wrench_sensor needs a backend with the batched joint reaction query (joint_reaction_forces); %s has none'
                                          % type(env.sim).__name__)
            w = env.sim.joint_reaction_forces(self.uid, self.frame_ids)
            B = w.shape[0]
            self._obs = OrderedDict(force=w[:, :, 0:3].reshape(B, -1).contiguous(), torque=w[:, :, 3:6].reshape(B, -1).contiguous())   # (copies: the backend reuses its output tensor)
            if self.use_motor_torque:
                self._obs['motor_torque'] = env.sim.joint_motor_torques(self.uid).clone()
            self._tick = env._tick
        return OrderedDict((k, env._out(v)) for k, v in self._obs.items())


class ImuSensor(Addon):
    """An inertial measurement unit on a model: what an accelerometer and a gyro mounted on one of its links read, by the batched
    link acceleration query (``env.sim.link_accelerations``; neither pybullet nor the reference has a counterpart).  The sensors a
    real quadrotor or wheeled robot flies and drives on, in place of the ground-truth world pose of ``object_state_sensor``.  Goes
    on a model.  Config keys: ``frame`` (a joint of the parent; default the base), ``xyz``, ``rpy`` (the mount in the URDF link
    frame, exactly ``camera``'s and ``lidar``'s keys and conventions), ``use_gravity`` False.

    * ``linear_acceleration`` ``[3]``: the specific force in sensor axes -- the sensor origin's acceleration over the last substep
      minus gravity; ``(0, 0, +|g|)`` at rest and level, zero in free fall but for the step's linear damping.
    * ``angular_velocity`` ``[3]``: in sensor axes.
    * ``gravity`` ``[3]`` (with ``use_gravity``): the unit gravity direction in sensor axes, ``(0, 0, -1)`` when level.

    ``compile()`` makes the scene keep the model's velocities at the start of the last substep
    (``builder.enable_joint_force_torque``).  Evaluated by ONE kernel launch of its own, lazily, the first time ``observe()`` is
    called after a step.  The readings are exact: noise and bias are the user's to add to the tensors."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        from ..mathx import quat_from_euler
        from ..model import Model
        if not isinstance(parent, Model):
            raise ValueError('imu_sensor goes on a model, not on the environment')
        self.uid = parent.uid
        self.frame_id = parent.get_frame_id(config.get('frame')) if 'frame' in config else -1
        if self.frame_id < 0 and 'frame' in config and config.get('frame') != 'base':
            raise ValueError('imu_sensor: model %r has no joint %r' % (parent.name, config.get('frame')))
        if parent.flat.fixed_base and len(parent.flat.links) == 0:
            raise ValueError('imu_sensor: model %r has a fixed base and no joints: it never moves and the scene keeps no velocities for it; '
                             'its reading would be the constant -g' % parent.name)
        self.local_pos = [float(v) for v in config.get('xyz', [0., 0., 0.])]
        self.local_orn = [float(v) for v in quat_from_euler(config.get('rpy', [0., 0., 0.]))]
        self.use_gravity = bool(config.get('use_gravity', False))
        box = lambda hi=np.inf: spaces.Box(-hi, hi, shape=(3, ), dtype='float32')
        sp = OrderedDict(linear_acceleration=box(), angular_velocity=box())
        if self.use_gravity:
            sp['gravity'] = box(1.)
        self.observation_space = spaces.Dict(sp)
        self.own_buffers = True   # like joint_wrench_sensor's, not part of the kernel's observation rows
        self._tick = None

    def compile(self, builder):
        builder.enable_joint_force_torque(self.uid)   # (the selector is a run-time argument of dg_world_link_accelerations)

    def observe(self):
        env = self.env
        if self._tick != env._tick:
            if not hasattr(env.sim, 'link_accelerations'):
                raise NotImplementedError('imu_sensor needs a backend with the batched link acceleration query (link_accelerations); %s has none'
                                          % type(env.sim).__name__)
            r = env.sim.link_accelerations(self.uid, [self.frame_id], self.local_pos, self.local_orn, com=False)
            self._obs = OrderedDict(linear_acceleration=r.specific_force[:, 0].contiguous(), angular_velocity=r.ang_vel[:, 0].contiguous())   # (copies: the backend reuses its output tensor)
            if self.use_gravity:
                self._obs['gravity'] = r.gravity[:, 0].contiguous()
            self._tick = env._tick
        return OrderedDict((k, env._out(v)) for k, v in self._obs.items())

"""The reference's ``ForceTorqueSensor`` and ``ElectricityCost`` written in plain Python against the batched second half of
``p.getJointStates`` -- ``env.sim.joint_reaction_forces`` and ``env.sim.joint_motor_torques`` -- the way a user of the reference ports
an addon of their own that reads ``jointReactionForces`` or ``appliedJointMotorTorque``.  tests/test_joint_wrench_gpu.py runs them."""
from collections import OrderedDict

from diy_gym_amd import spaces
from diy_gym_amd.addons.addon import Addon


class PyForceTorqueSensor(Addon):
    """The reference's ``ForceTorqueSensor`` (diy_gym/addons/sensors/force_torque_sensor.py:7-23) line by line, batched:
    ``p.enableJointForceTorqueSensor`` at construction -> ``builder.enable_joint_force_torque`` in ``compile()`` (the one thing that
    must happen while the scene is built: the step then keeps the model's velocities at the start of its last substep),
    ``p.getJointState(uid, frame)[2]`` -> ``sim.joint_reaction_forces(uid, [frame])``."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        self.uid = parent.uid
        self.frame_id = parent.get_frame_id(config.get('frame')) if 'frame' in config else -1
        box = lambda: spaces.Box(-10, 10, shape=(3, ), dtype='float32')
        self.observation_space = spaces.Dict(OrderedDict(force=box(), torque=box()))
        self.own_buffers = True   # its observation is not part of the kernel's observation rows

    def compile(self, builder):
        builder.enable_joint_force_torque(self.uid)

    def observe(self):
        state = self.env.sim.joint_reaction_forces(self.uid, [self.frame_id])[:, 0]
        return OrderedDict(force=state[:, :3].clone(), torque=state[:, 3:].clone())


class PyElectricityCost(Addon):
    """The reference's ``ElectricityCost`` (diy_gym/addons/rewards/electricity_cost.py:7-18): ``getJointStates(..)[3]`` ->
    ``sim.joint_motor_torques``, ``[1]`` -> ``sim.joint_states`` (fixed base) or the rates a floating body's sensor reports."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        self.uid = parent.uid
        self.multiplier = config.get('multiplier', 1.0)

    def reward(self):
        torque = self.env.sim.joint_motor_torques(self.uid)
        velocity = self.env.sim.joint_states(self.uid)[1]
        return -(torque * velocity).abs().sum(dim=1) * self.multiplier

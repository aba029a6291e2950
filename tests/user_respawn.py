"""The reference's ``Respawn`` written in plain Python against the batched ``env.sim.reset_base_state`` -- the first thing a user of
the reference writes when the compiled ``respawn`` (uniform jitter about the load pose) is not the distribution they want: a
curriculum, a scripted placement, a replay of recorded initial conditions.  No ``compile()``: the environment calls ``reset()`` before
every reset, with the mask of the reset in progress in ``env.reset_mask``.  tests/test_state_io_gpu.py runs it."""
import torch

from diy_gym_amd.addons.addon import Addon
from user_ik_controller import quaternion_from_euler, quaternion_multiply


class PyRespawn(Addon):
    """The reference's ``Respawn`` (diy_gym/addons/misc/respawn.py:7-39) line by line, batched: ``p.getBasePositionAndOrientation``
    at construction -> the model's load pose, ``np.random.random`` -> a seeded ``torch.Generator`` (config key ``seed``), one draw per
    env, ``p.resetBasePositionAndOrientation`` -> ``sim.reset_base_state`` under ``env.reset_mask``.  The model must be one whose base
    the scene lets move: a floating base, or a fixed one that also carries the compiled ``respawn``."""
    def __init__(self, parent, config):
        super().__init__(parent, config)
        self.uid = parent.uid
        self.initial_pose = (torch.tensor(parent.position, dtype=torch.float32), torch.tensor(parent.orientation, dtype=torch.float32))
        self.position_range = torch.tensor(config.get('position_range', [0., 0., 0.]), dtype=torch.float32)
        self.rotation_range = torch.tensor(config.get('rotation_range', [0., 0., 0.]), dtype=torch.float32)
        self.once = config.get('once', False)
        self.generator = torch.Generator().manual_seed(int(config.get('seed', 0)))
        self.pose = None   # (the reference draws in its constructor; here the batch size is known at the first reset)

    def generate_pose(self):
        B = self.env.sim.num_envs
        pos = (torch.rand((B, 3), generator=self.generator) - 0.5) * self.position_range + self.initial_pose[0]
        rpy = (torch.rand((B, 3), generator=self.generator) - 0.5) * self.rotation_range
        return pos, quaternion_multiply(self.initial_pose[1].reshape(1, 4).expand(B, 4), quaternion_from_euler(rpy))

    def reset(self):
        if not self.once or self.pose is None:
            self.pose = self.generate_pose()
        self.env.sim.reset_base_state(self.uid, pos=self.pose[0], orn=self.pose[1], mask=self.env.reset_mask)

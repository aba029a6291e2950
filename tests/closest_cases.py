"""The cases the closest-points tests share: which scene, how its state is reached, which queries are asked.  tests/test_closest_ref.py
checks on the CPU that every case is what it claims (pairs within and beyond the distance, nothing near the threshold, ...);
tests/test_closest_gpu.py runs the same cases on the GPU against the same reference figures, computed once per (case, batch)."""
import collections
import functools
import os
import sys

import numpy as np

import closest_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, GOLDEN)   # make_vectors: the pressed-together inputs of the arms

BATCHES = (1, 3, 70)   # one lane; a wavefront with a partial tail; more than one wavefront
# no asserted pair may lie this close to the query's `distance`, and the nearest pair must lead the runner-up by this much: far
# above any fp32 error of a distance (the contact query's is 2.3e-7 m), far below the spacing of the scenes' pairs
CLEAR = 1e-4

# scene, engine overrides, steps, scale of the seeded random actions (None: the arms' pressing inputs), and the queries
# (model A, model B or None, distance); `pruned`: the case claims a statically pruned pair within the distance
Case = collections.namedtuple('Case', ['scene', 'engine', 'steps', 'scale', 'queries', 'pruned'])
CASES = {
    'marbles': Case('contacts_marbles', {}, 40, 60.0, (('red_marble', None, 0.5), ('blue_marble', None, 0.4)), False),
    'box_stack': Case('contacts_box_stack', {}, 10, 0.0, (('upper', None, 0.05), ('plane', None, 0.05)), False),
    'r2d2': Case('contacts_r2d2', {}, 10, 0.0, (('r2d2', None, 0.1), ('plane', 'r2d2', 0.15)), False),
    'arms': Case('contacts_arms', {}, 15, None, (('ur5_l', 'ur5_r', 0.157), ('ur5_r', None, 0.9)), True),
    'two_arms': Case('np_two_arms', {}, 3, 0.0, (('arm_a', 'arm_b', 0.05), ), True),
    'arms_capsules': Case('contacts_arms', {'hull_contacts': 0}, 15, None, (('ur5_l', 'ur5_r', 0.1), ), False),
}
GEOMETRY = ('marbles', 'box_stack', 'r2d2', 'arms')   # sphere-sphere / sphere-box, hull-box / hull-hull, capsule / hull on box, hull-hull


def path(name):
    for p in (os.path.join(GOLDEN, name + '.yaml'), os.path.join(GOLDEN, 'proximity_sensor', name + '.yaml')):
        if os.path.isfile(p):
            return p
    raise KeyError(name)


def cpu_env(scene, B, engine=None, **kw):
    from diy_gym_amd import DIYGym
    return DIYGym(path(scene), num_envs=B, seed=5, backend_factory=closest_ref.ClosestOracleBackend, **({'engine': engine} if engine else {}), **kw)


def gpu_env(scene, B, engine=None, **kw):
    from diy_gym_amd import DIYGym
    return DIYGym(path(scene), num_envs=B, seed=5, device='cuda:0', **({'engine': engine} if engine else {}), **kw)


def actions_of(env, case):
    import torch
    if case.scale is None:
        import make_vectors
        return make_vectors.press_actions(env, case.steps)
    gen = torch.Generator().manual_seed(11)
    return (torch.rand((case.steps, env.num_envs, max(env.layout.act_dim, 1)), generator=gen) * 2 - 1) * case.scale


Reference = collections.namedtuple('Reference', ['state', 'layout', 'uids', 'answers', 'poses', 'ref'])


@functools.lru_cache(maxsize=None)
def reference(name, B):
    """The checker's state after the case's steps and, per query, every candidate pair measured in fp64 -- computed once per
    (case, batch) and never written to."""
    case = CASES[name]
    cpu = cpu_env(case.scene, B, case.engine); acts = actions_of(cpu, case)
    for s in range(case.steps):
        cpu.sim.step(cpu._all_slots, acts[s])
    ref = closest_ref.ClosestRef(cpu.layout)
    uids = {k: m.uid for k, m in cpu.models.items()}
    answers, poses = [], None
    for a, b, dist in case.queries:
        measured, poses = ref.measure(cpu.sim, uids[a], None if b is None else uids[b])
        answers.append((uids[a], None if b is None else uids[b], dist, measured))
    return Reference(cpu.sim.get_state(), cpu.layout, uids, answers, poses, ref)


def rows_of(measured, distance):
    return [[p for p in env if p.distance < distance] for env in measured]


def nearest_of(rows):
    out = []
    for r in rows:
        best = None
        for p in r:
            if best is None or p.distance < best.distance:
                best = p
        out.append(best)
    return out

"""Reference for the batched contact query (``dg_world_contacts`` / ``env.sim.contact_points``): the contact list of the fp64
checker's most recent substep, in the query's own form.

The checker (oracle/dgsim_oracle.c) keeps, per env, the contacts of the last substep it ran: point, normal from B towards A,
signed distance and the normal impulse its solver ended with (``OracleBackend.contacts`` / ``contact``).  The query reports the
contacts AT the state it is handed.  The two describe the same thing when the scene runs ONE substep per step and the state is the
one the checker's step started from: ``cpu.set_state(S); cpu.step(zero action)`` makes the checker's list the contacts at S.  The
checker has no ids (it reports no pair), so ``id_a`` / ``id_b`` are None; ids are tested against known answers."""
import collections

import numpy as np

ContactPoints = collections.namedtuple('ContactPoints', ['count', 'id_a', 'id_b', 'pos_a', 'pos_b', 'normal', 'distance', 'normal_force'])


def oracle_contact_points(cpu_env, capacity=None):
    """``ContactPoints`` (numpy, fp64) of the checker's last substep for every env of ``cpu_env`` (a DIYGym on the OracleBackend):
    ``pos_a`` / ``pos_b`` = point +/- normal x distance / 2, ``normal_force`` = impulse / substep length.  ``capacity``: the C of
    the arrays (default: the scene's ``max_contacts``); slots behind an env's count are zero."""
    sim, B = cpu_env.sim, cpu_env.num_envs
    C = int(cpu_env.layout.max_contacts) if capacity is None else int(capacity)
    h = float(cpu_env.layout.dt)
    count = np.zeros(B, dtype=np.int32)
    pos_a, pos_b, normal = (np.zeros((B, C, 3)) for _ in range(3))
    distance, force = np.zeros((B, C)), np.zeros((B, C))
    for e in range(B):
        count[e] = sim.contacts(e)
        assert count[e] <= C, (e, count[e], C)
        for k in range(count[e]):
            c = np.asarray(sim.contact(e, k), dtype=np.float64)
            p, n, d = c[0:3], c[3:6], c[6]
            pos_a[e, k], pos_b[e, k], normal[e, k], distance[e, k], force[e, k] = p + n * (0.5 * d), p - n * (0.5 * d), n, d, c[7] / h
    return ContactPoints(count, None, None, pos_a, pos_b, normal, distance, force)

"""Reference for the contact-force queries (``dg_world_contact_forces`` / ``dg_world_net_contact_wrench``): every output restated
in numpy fp64 from a contact list and a contact impulse cache.

Two sources feed the same restatement:

* the fp64 checker -- ``cpu.set_state(S); cpu.step(zero action)`` on a scene with ONE substep per step leaves the contact list AT
  S in ``sim.contact(e, k)`` and, in the checker's state at the layout's ``warm_off``, the cache ``[count][key normal t1 t2]``
  whose entry k belongs to contact k (``oracle_contact_forces``);
* the GPU's own numbers -- the cache read from ``env.sim.get_state()`` and the geometry from ``contact_points``
  (``restate_from_query``), which pins the readout kernel to the bit where it copies and to fp32 rounding where it computes.

A contact's pair is ``key // 256`` (DG_CONTACT_KEY); the pair's two shapes give ids, links and the friction coefficient."""
import collections

import numpy as np

from diy_gym_amd.scene import K

Contact = collections.namedtuple('Contact', ['pair', 'id_a', 'id_b', 'pos_a', 'pos_b', 'normal', 'normal_force', 'lateral_friction1', 'lateral_dir1',
                                             'lateral_friction2', 'lateral_dir2', 'force_on_a', 'mu'])


def tangent_basis(n):
    """``tangent_basis`` of dg_solver.h in fp64: the two unit tangents of the friction rows of a contact with unit normal ``n``."""
    n = np.asarray(n, dtype=np.float64)
    if abs(n[2]) > 0.70710678118654752:
        a = n[1] * n[1] + n[2] * n[2]; k = 1.0 / np.sqrt(a)
        t1 = np.array([0.0, -n[2] * k, n[1] * k]); t2 = np.array([a * k, -n[0] * t1[2], n[0] * t1[1]])
    else:
        a = n[0] * n[0] + n[1] * n[1]; k = 1.0 / np.sqrt(a)
        t1 = np.array([-n[1] * k, n[0] * k, 0.0]); t2 = np.array([-n[2] * t1[1], n[2] * t1[0], a * k])
    return t1, t2


class Tables:
    """The layout's shape and pair tables: per pair the two shapes' ids (uid + ((link + 1) << 24)) and the friction product."""
    def __init__(self, layout):
        I, F = layout.I, layout.F
        ns, npairs = int(I[K.H_N_SHAPES]), int(I[K.H_N_PAIRS])
        SI = I[I[K.H_OFF_SHAPE_I]:I[K.H_OFF_SHAPE_I] + ns * K.SI_STRIDE].reshape(ns, K.SI_STRIDE)
        SF = F[I[K.H_OFF_SHAPE_F]:I[K.H_OFF_SHAPE_F] + ns * K.SF_STRIDE].reshape(ns, K.SF_STRIDE)
        PI = I[I[K.H_OFF_PAIR_I]:I[K.H_OFF_PAIR_I] + npairs * K.PI_STRIDE].reshape(npairs, K.PI_STRIDE)
        shape_id = SI[:, K.SI_BODY] + (((SI[:, K.SI_FLAGS] >> 8) & 0xFFFF) << 24)
        self.pair_ids = np.stack([shape_id[PI[:, K.PI_A]], shape_id[PI[:, K.PI_B]]], axis=1).astype(np.int64)
        # CL_MU of build_contact_rows: the product of the two shapes' friction, in fp32 as the kernel forms it
        fr = SF[:, K.SF_FRICTION].astype(np.float32)
        self.pair_mu = (fr[PI[:, K.PI_A]] * fr[PI[:, K.PI_B]]).astype(np.float32)
        self.h = float(layout.dt)
        self.warm_off = int(layout.warm_off)
        self.max_contacts = int(layout.max_contacts)


def cache_of(state_row, tables):
    """``(keys [n], impulses [n, 3])`` of one env's contact impulse cache."""
    w = tables.warm_off
    n = int(state_row[w])
    rows = np.asarray(state_row[w + 1:w + 1 + n * K.WS_STRIDE], dtype=np.float64).reshape(n, K.WS_STRIDE)
    return rows[:, K.WS_KEY].astype(np.int64), rows[:, K.WS_NORMAL:K.WS_NORMAL + 3]


def make_contact(tables, pair, p_a, p_b, n, forces):
    """One contact in the narrow phase's own orientation (A, B of the pair), every output in fp64."""
    n = np.asarray(n, dtype=np.float64); t1, t2 = tangent_basis(n); fn, f1, f2 = (float(x) for x in forces)
    ia, ib = (int(x) for x in tables.pair_ids[pair])
    return Contact(pair, ia, ib, np.asarray(p_a, dtype=np.float64), np.asarray(p_b, dtype=np.float64), n, fn, f1, t1, f2, t2, fn * n + f1 * t1 + f2 * t2,
                   float(tables.pair_mu[pair]))


def swapped(c):
    """The contact seen from its B side: the swap rule -- ids and points exchanged, normal and BOTH tangents negated, scalars kept."""
    return c._replace(id_a=c.id_b, id_b=c.id_a, pos_a=c.pos_b, pos_b=c.pos_a, normal=-c.normal, lateral_dir1=-c.lateral_dir1, lateral_dir2=-c.lateral_dir2,
                      force_on_a=-c.force_on_a)


def id_matches(i, body, link):
    return body is None or ((i & 0xFFFFFF) == body and (link is None or (i >> 24) - 1 == link))


def filtered(contacts, body_a=None, link_a=None, body_b=None, link_b=None):
    """The rows a query with these filters reports, in order, with the side swapping of contact_query_kernel."""
    out = []
    for c in contacts:
        fwd = id_matches(c.id_a, body_a, link_a) and id_matches(c.id_b, body_b, link_b)
        rev = id_matches(c.id_b, body_a, link_a) and id_matches(c.id_a, body_b, link_b)
        if fwd or rev:
            out.append(c if fwd else swapped(c))
    return out


def net_wrench(contacts, body, link, origin, body_b=None, link_b=None):
    """``(force 3, moment 3 about origin, count)`` of the contacts that have (body, link) on a side."""
    rows = filtered(contacts, body, link, body_b, link_b)
    F, T = np.zeros(3), np.zeros(3)
    for c in rows:
        F += c.force_on_a; T += np.cross(c.pos_a - np.asarray(origin, dtype=np.float64), c.force_on_a)
    return F, T, len(rows)


def oracle_contact_forces(cpu_env):
    """Per env the contact list of the checker's last substep with the forces of its own cache (entry k for contact k)."""
    sim, tables = cpu_env.sim, Tables(cpu_env.layout)
    S = sim.get_state(); out = []
    for e in range(cpu_env.num_envs):
        keys, imp = cache_of(S[e], tables)
        assert len(keys) == sim.contacts(e), (e, len(keys), sim.contacts(e))
        env = []
        for k in range(len(keys)):
            c = sim.contact(e, k); p, n, d = c[0:3], c[3:6], c[6]
            assert abs(imp[k, 0] - c[7]) == 0.0, (e, k)   # the cache's normal impulse is the one the checker reports for contact k
            env.append(make_contact(tables, int(keys[k]) // 256, p + n * (0.5 * d), p - n * (0.5 * d), n, imp[k] / tables.h))
        out.append(env)
    return out


def restate_from_query(cp, state, layout):
    """Per env the contacts of an UNFILTERED ``contact_points`` answer ``cp`` (numpy) with the forces of the cache in ``state``
    (numpy ``[B, state_dim]``, fp32): a row takes the first unused cache entry of a pair with its ids whose normal impulse gives the
    row's normal force bits, and zeros when there is none (a contact the cache does not know).  The scalars are formed as the kernel
    forms them, ``float32(impulse) * (float32(1) / float32(h))``; everything derived from them is fp64.  Also returns, per env, the
    number of rows that found an entry."""
    tables = Tables(layout); inv_h = np.float32(1.0) / np.float32(tables.h); out, found = [], []
    for e in range(len(cp.count)):
        keys, imp = cache_of(state[e], tables); imp32 = imp.astype(np.float32); used = np.zeros(len(keys), dtype=bool); env = []; hit = 0
        for k in range(int(cp.count[e])):
            ids = (int(cp.id_a[e, k]), int(cp.id_b[e, k])); pick = None
            for j in range(len(keys)):
                pair = int(keys[j]) // 256
                if not used[j] and tuple(tables.pair_ids[pair]) == ids and (imp32[j, 0] * inv_h).view(np.int32) == cp.normal_force[e, k].view(np.int32):
                    pick = j
                    break
            if pick is None:
                pair = int(np.nonzero((tables.pair_ids == ids).all(1))[0][0]); f = np.zeros(3, dtype=np.float32)
            else:
                used[pick] = True; hit += 1; pair = int(keys[pick]) // 256; f = imp32[pick] * inv_h
            env.append(make_contact(tables, pair, cp.pos_a[e, k], cp.pos_b[e, k], cp.normal[e, k], f))
        out.append(env); found.append(hit)
    return out, found


def damping_force(layout, m, v):
    """The checker's velocity damping of a free body whose centre of mass is its origin (damping_force in oracle/dgsim_oracle.c):
    ``-m v (k + k |v|)`` with k = the scene's linear damping, applied as a force at the velocity the step starts from."""
    k = float(layout.F[K.HF_LIN_DAMPING]); v = np.asarray(v, dtype=np.float64)
    return -m * v * (k + k * np.linalg.norm(v, axis=-1, keepdims=True))


def gravity(layout):
    return np.array([layout.F[K.HF_GRAV_X], layout.F[K.HF_GRAV_Y], layout.F[K.HF_GRAV_Z]], dtype=np.float64)

"""CPU reference of the whole-arm contact of the simulated plant (include/sai2b.h "whole-arm contact"; numpy float64,
no GPU; test infrastructure). It builds on collision_reference.CollisionReference: the spheres, the masks, the link of every
sphere and the URDF chain (tests/urdf_np.Chain, an independent reading of the URDF) are that object's. The chain is walked here
once more with the whole batch in every array, because a period asks for the kinematics of every robot at every substep;
tests/test_body_contact_reference.py holds this walk to CollisionReference.centres / point_jacobian robot by robot.

The law is written candidate by candidate in the order of the specification, every tested candidate contributes, and the joint
torques are tb = sum J_c^T F with the explicit point Jacobian J_c [3][n] of every application point: deliberately not the
kernel's per-sphere wrench and projection. One substep is

    forces(q, dq)["tau"] = tb  ->  Oracle.sim_step(tau + tc + tb, h, 1)

and a period of s substeps is s such calls (tc: a ContactReference's, when given). With joint dynamics the step is
JointDynamicsReference's, which takes the sum through its contact= hook (Sum below, as external_wrench_reference.Combined)."""
import numpy as np

import oracle_lib as ol
from collision_reference import CATEGORIES, CollisionReference

PLANE, OBSTACLE, SELF = 1, 2, 4
ALL = PLANE | OBSTACLE | SELF


def _skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def point_force(u, delta, v, k, d, mu, v_eps):
    """u, v [B][3], delta, k, d, mu [B] -> f_n [B], F [B][3]: the plant's contact law term for term. np.fmax drops a NaN as the
    C fmax does; a robot whose rows are not all >= 0 (a NaN compares false) feels nothing"""
    with np.errstate(invalid="ignore"):
        ok = (k >= 0) & (d >= 0) & (mu >= 0)
        k, d, mu = np.where(ok, k, 0.0), np.where(ok, d, 0.0), np.where(ok, mu, 0.0)
        vn = np.sum(u * v, axis=1)
        fn = np.fmax(0.0, k * np.fmax(0.0, delta) * (1.0 - d * vn))
        vt = v - vn[:, None] * u
        F = fn[:, None] * u - (mu * fn / np.sqrt(np.sum(vt * vt, axis=1) + v_eps * v_eps))[:, None] * vt
        on = fn > 0
        return np.where(on, fn, 0.0), np.where(on[:, None], F, 0.0)


class BodyContactReference:
    def __init__(self, collision: CollisionReference, model, B, rows, categories=ALL, v_eps=1e-3, plant=None, contact=None, threads=8):
        """collision: the CollisionReference whose geometry is the body; rows [3][B]: k, d, mu; plant: an object with set_state /
        get_state / sim_step over the batch (default: an Oracle of `model`); contact: a ContactReference (its tau is tc)"""
        self.col, self.B, self.dof = collision, B, int(model.dof)
        self.rows = np.array(rows, dtype=np.float64)
        assert self.rows.shape == (3, B)
        self.categories, self.v_eps = int(categories), float(v_eps)
        self.plant = plant if plant is not None else ol.Oracle(model, [ol.joint_task("j", robot_dof=self.dof)], B, threads=threads)
        self.contact = contact
        self.env = None  # [6 P + 4 O][B], read at every evaluation: the caller may move an obstacle between two steps

    # ---- the chain, batched
    def kinematics(self, q):
        """q [n][B] -> x [S][B][3] world centres, links [S], axes [n][B][3], origins [n][B][3], types [n] ('prismatic' | other)"""
        ch, B = self.col.chain, q.shape[1]
        pb, Rb = self.col.base
        out = {ch.root: (np.broadcast_to(np.eye(3), (B, 3, 3)), np.zeros((B, 3)), -1)}
        axes, origins, types = [None] * ch.dof, [None] * ch.dof, [None] * ch.dof
        cur = [ch.root]
        while cur:
            nxt = []
            for j in ch.joints:
                if j["parent"] not in cur:
                    continue
                Rp, pp, mv = out[j["parent"]]
                R, p = Rp @ j["R"], pp + Rp @ j["xyz"]
                if j["type"] != "fixed":
                    k = ch.moving.index(j)
                    a = j["axis"] / np.linalg.norm(j["axis"])
                    aw = R @ a
                    if j["type"] == "prismatic":
                        p = p + aw * q[k][:, None]
                    else:
                        K = _skew(a)
                        s, c = np.sin(q[k])[:, None, None], np.cos(q[k])[:, None, None]
                        R = R @ (np.eye(3) + s * K + (1.0 - c) * (K @ K))
                    axes[k], origins[k], types[k], mv = aw @ Rb.T, pb + p @ Rb.T, j["type"], k
                out[j["child"]] = (R, p, mv)
                nxt.append(j["child"])
            cur = nxt
        x = []
        for name, c, _ in self.col.spheres:
            if name is None:
                x.append(np.broadcast_to(c, (B, 3)).copy())
            else:
                R, p, _ = out[name]
                x.append(pb + (p + R @ c) @ Rb.T)
        return np.array(x), list(self.col.links), axes, origins, types

    @staticmethod
    def _jacobian(c, link, axes, origins, types):
        """d c / d q [B][3][n] of the material point of moving link `link` (-1: the world) that stands at c [B][3]"""
        B, n = c.shape[0], len(axes)
        J = np.zeros((B, 3, n))
        for m in range(link + 1):
            J[:, :, m] = axes[m] if types[m] == "prismatic" else np.cross(axes[m], c - origins[m])
        return J

    # ---- the law
    def forces(self, q, dq, env=None):
        """-> dict tau [n][B] = tb, depth [3][B], index [3][B], normal_force [3][B] (sum of f_n), power [B] = sum F . v_rel,
        candidates: [(category, index, delta [B], fn [B], F [B][3])] for every tested candidate, active [B]: candidates with
        f_n > 0"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self._forces(np.asarray(q, dtype=np.float64), np.asarray(dq, dtype=np.float64), self.env if env is None else env)

    def _forces(self, q, dq, env):
        col, B, n = self.col, self.B, self.dof
        k, d, mu = self.rows
        x, links, axes, origins, types = self.kinematics(q)
        r = [s[2] for s in col.spheres]
        S = len(r)
        dqT = dq.T
        tb = np.zeros((B, n))
        depth, index, fsum = np.zeros((3, B)), np.full((3, B), -1.0), np.zeros((3, B))
        power, active, cands = np.zeros(B), np.zeros(B, dtype=int), []

        def note(cat, idx, delta, fn, F):
            wins = delta > depth[cat]  # the first strict maximum in the law's order: of equally deep ones the smallest index
            depth[cat], index[cat] = np.where(wins, delta, depth[cat]), np.where(wins, idx, index[cat])
            fsum[cat] += fn
            active[:] += fn > 0
            cands.append((CATEGORIES[cat], idx, delta, fn, F))

        if self.categories & PLANE:
            for p in range(col.P):
                p0, nrm = env[6 * p : 6 * p + 3].T, env[6 * p + 3 : 6 * p + 6].T
                for kk in range(S):
                    if (col.env_mask >> kk) & 1:
                        delta = r[kk] - np.sum(nrm * (x[kk] - p0), axis=1)
                        c = x[kk] - r[kk] * nrm
                        J = self._jacobian(c, links[kk], axes, origins, types)
                        v = np.einsum("bin,bn->bi", J, dqT)
                        fn, F = point_force(nrm, delta, v, k, d, mu, self.v_eps)
                        tb += np.einsum("bin,bi->bn", np.where((fn > 0)[:, None, None], J, 0.0), F)
                        power += np.where(fn > 0, np.sum(F * v, axis=1), 0.0)
                        note(0, 16 * p + kk, delta, fn, F)
        if self.categories & OBSTACLE:
            for o in range(col.O):
                w = env[6 * col.P + 4 * o : 6 * col.P + 4 * o + 4]
                for kk in range(S):
                    if (col.env_mask >> kk) & 1:
                        e = x[kk] - w[:3].T
                        norm = np.linalg.norm(e, axis=1)
                        some = norm > 0
                        u = np.where(some[:, None], e / np.where(some, norm, 1.0)[:, None], 0.0)
                        delta = np.where(some, r[kk] + w[3] - norm, 0.0)
                        c = x[kk] - r[kk] * u
                        J = self._jacobian(c, links[kk], axes, origins, types)
                        v = np.einsum("bin,bn->bi", J, dqT)
                        fn, F = point_force(u, delta, v, k, d, mu, self.v_eps)
                        tb += np.einsum("bin,bi->bn", np.where((fn > 0)[:, None, None], J, 0.0), F)
                        power += np.where(fn > 0, np.sum(F * v, axis=1), 0.0)
                        note(1, 16 * o + kk, delta, fn, F)
        if self.categories & SELF:
            for i in range(S):
                for j in range(i + 1, S):
                    if (col.pair_mask[i] >> j) & 1:
                        e = x[i] - x[j]
                        norm = np.linalg.norm(e, axis=1)
                        some = norm > 0
                        u = np.where(some[:, None], e / np.where(some, norm, 1.0)[:, None], 0.0)
                        delta = np.where(some, r[i] + r[j] - norm, 0.0)
                        ci, cj = x[i] - r[i] * u, x[j] + r[j] * u
                        Ji = self._jacobian(ci, links[i], axes, origins, types)
                        Jj = self._jacobian(cj, links[j], axes, origins, types)
                        v = np.einsum("bin,bn->bi", Ji - Jj, dqT)
                        fn, F = point_force(u, delta, v, k, d, mu, self.v_eps)
                        tb += np.einsum("bin,bi->bn", np.where((fn > 0)[:, None, None], Ji - Jj, 0.0), F)
                        power += np.where(fn > 0, np.sum(F * v, axis=1), 0.0)
                        note(2, 16 * i + j, delta, fn, F)
        return dict(tau=np.ascontiguousarray(tb.T), depth=depth, index=index, normal_force=fsum, power=power, candidates=cands,
                    active=active, centres=x)

    # ---- the plant
    def set_state(self, q, dq):
        self.plant.set_state(np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(dq, dtype=np.float64))
        if self.contact is not None and self.contact.plant is not self.plant:
            self.contact.set_state(q, dq)

    def get_state(self):
        return self.plant.get_state()

    def step(self, tau, dt=0.001, substeps=1, with_gravity=False, watch=None):
        """one control period of the plain step under the held torques tau [n][B] (None: zero). watch: a list that receives
        forces() of every substep"""
        tau = np.zeros((self.dof, self.B)) if tau is None else np.asarray(tau, dtype=np.float64)
        h = dt / substeps
        for _ in range(substeps):
            q, dq = self.plant.get_state()
            f = self.forces(q, dq)
            if watch is not None:
                watch.append(f)
            t = tau + self.contact.forces(q, dq)["tau"] if self.contact is not None else tau
            self.plant.sim_step(np.ascontiguousarray(t + f["tau"]), h, 1, bool(with_gravity))
        if self.contact is not None and self.contact.plant is not self.plant:
            self.contact.set_state(*self.plant.get_state())

    def report(self, q=None, dq=None):
        """what the kernel reports after the last substep -> dict status [9 + n][B], counts [4]"""
        if q is None:
            q, dq = self.plant.get_state()
        f = self.forces(q, dq)
        touching = f["normal_force"] > 0
        return dict(status=np.concatenate([f["depth"], f["index"], f["normal_force"], f["tau"]]),
                    counts=[int(touching[c].sum()) for c in range(3)] + [int(touching.any(axis=0).sum())], forces=f)


class Sum:
    """what JointDynamicsReference (and ExternalWrenchReference) take through their contact= hook: forces(q, dq)["tau"] = the
    sum of the parts' (a BodyContactReference, a ContactReference, an external_wrench_reference.Combined)"""

    def __init__(self, *parts):
        self.parts = [p for p in parts if p is not None]
        self.plant = None

    def forces(self, q, dq):
        return dict(tau=sum(p.forces(q, dq)["tau"] for p in self.parts))

    def set_state(self, q, dq):
        for p in self.parts:
            if hasattr(p, "set_state"):
                p.set_state(q, dq)

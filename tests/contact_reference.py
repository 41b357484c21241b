"""CPU reference of the contact model of the simulated plant (DESIGN "Contact in the simulated plant"; numpy float64, no
GPU; test infrastructure). One substep is

    Oracle.set_state -> pose and Jacobian of the contact link from the oracle (a one-task oracle context whose
    MotionForceTask sits at the link origin: x_k = pos + R c_k, J_k = J_v - [R c_k]x J_w) -> the force law below in
    numpy -> Oracle.sim_step(tau + sum_k J_k^T F_k, h, 1)

and a period of s substeps is s such calls. The sensor and status rows come from the final state the same way. The oracle is
used through its existing entry points only; the plant may be any object with set_state / get_state / sim_step over the
batch (oracle_lib.Oracle, or payload_cases.PayloadOracles for a plant whose robots carry payloads)."""
import numpy as np

import oracle_lib as ol

MAX_POINTS = 4


def force_law(x, v, rows, v_eps):
    """x, v [3][B] of one point, rows [9][B] (plane point 3, unit normal 3, k, d, mu) -> delta [B], f_n [B], F [3][B]:
        delta = n . (p0 - x),  vn = n . v,  f_n = max(0, k max(0, delta) (1 - d vn)),  v_t = v - vn n,
        F = f_n n - mu f_n v_t / sqrt(|v_t|^2 + v_eps^2)         (the force ON the robot, world frame)"""
    p0, n, k, d, mu = rows[0:3], rows[3:6], rows[6], rows[7], rows[8]
    delta = np.sum(n * (p0 - x), axis=0)
    vn = np.sum(n * v, axis=0)
    fn = np.maximum(0.0, k * np.maximum(0.0, delta) * (1.0 - d * vn))
    vt = v - vn * n
    F = fn * n - mu * fn * vt / np.sqrt(np.sum(vt * vt, axis=0) + v_eps * v_eps)
    return delta, fn, F


def _cross(a, b):
    return np.cross(a, b, axis=0)


class ContactReference:
    def __init__(self, model, B, link, points, rows, v_eps=1e-3, plant=None, threads=8):
        self.dof, self.B, self.link = int(model.dof), B, int(link)
        self.points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        assert 1 <= len(self.points) <= MAX_POINTS
        self.rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert self.rows.shape == (9, B)
        self.v_eps = float(v_eps)
        at_origin = ol.motion_force_task("contact_link", link=self.link, frame_pos=(0.0, 0.0, 0.0), robot_dof=self.dof)
        self.kin = ol.Oracle(model, [at_origin], B, threads=threads)
        self.plant = plant if plant is not None else ol.Oracle(model, [at_origin], B, threads=threads)

    # -- kinematics of the points, from the oracle
    def point_kinematics(self, q, dq):
        """-> x [K][3][B], J [K][3][n][B] (linear Jacobians), v [K][3][B]"""
        n, B = self.dof, self.B
        self.kin.set_state(q, dq)
        _, J, pos, rot = self.kin.get_model(0)
        J = J.reshape(6, n, B)
        R = rot.reshape(3, 3, B)
        xs, Js, vs = [], [], []
        for c in self.points:
            r = np.einsum("ijb,j->ib", R, c)  # R c_k
            Jk = J[:3] - np.stack([_cross(r, J[3:, i]) for i in range(n)], axis=1)  # J_v - [r]x J_w
            xs.append(pos + r)
            Js.append(Jk)
            vs.append(np.einsum("inb,nb->ib", Jk, dq))
        return np.stack(xs), np.stack(Js), np.stack(vs)

    def forces(self, q, dq):
        """-> dict x, v, F [K][3][B], delta, fn [K][B], tau [n][B] = sum_k J_k^T F_k"""
        x, J, v = self.point_kinematics(q, dq)
        K = len(self.points)
        delta, fn, F = np.empty((K, self.B)), np.empty((K, self.B)), np.empty((K, 3, self.B))
        tau = np.zeros((self.dof, self.B))
        for k in range(K):
            delta[k], fn[k], F[k] = force_law(x[k], v[k], self.rows, self.v_eps)
            tau += np.einsum("inb,ib->nb", J[k], F[k])
        return dict(x=x, v=v, F=F, delta=delta, fn=fn, tau=tau)

    # -- the plant
    def set_state(self, q, dq):
        self.plant.set_state(np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(dq, dtype=np.float64))

    def get_state(self):
        return self.plant.get_state()

    def step(self, tau, dt=0.001, substeps=1, with_gravity=False):
        """one control period under the held torques tau [n][B] (None: zero)"""
        tau = np.zeros((self.dof, self.B)) if tau is None else np.asarray(tau, dtype=np.float64)
        h = dt / substeps
        for _ in range(substeps):
            q, dq = self.plant.get_state()
            f = self.forces(q, dq)
            self.plant.sim_step(np.ascontiguousarray(tau + f["tau"]), h, 1, bool(with_gravity))

    # -- what the kernel reports after the last substep
    def report(self, sensor=None):
        """sensor: None, or (oracle with the controller's hierarchy, task index): its control point x_c and frame R_c are read at
        the plant's current state, its sensor_rot / sensor_pos from its config. Without one x_c is the contact link's origin.
        -> dict depth, normal_force [4][B], wrench_world [6][B], robots_in_contact, sensed [6][B] (None without a sensor)"""
        q, dq = self.plant.get_state()
        f = self.forces(q, dq)
        B, K = self.B, len(self.points)
        depth, nf = np.zeros((MAX_POINTS, B)), np.zeros((MAX_POINTS, B))
        depth[:K], nf[:K] = f["delta"], f["fn"]
        if sensor is None:
            _, _, xc, _ = self.kin.get_model(0)
        else:
            o, task = sensor
            o.set_state(q, dq)
            _, _, xc, Rc = o.get_model(task)
        Ft = f["F"].sum(axis=0)
        Mt = sum(_cross(f["x"][k] - xc, f["F"][k]) for k in range(K))
        out = dict(depth=depth, normal_force=nf, wrench_world=np.concatenate([Ft, Mt]),
                   robots_in_contact=int(np.count_nonzero((nf > 0).any(axis=0))), sensed=None)
        if sensor is not None:
            cfg = o.tasks[task]
            Rc = Rc.reshape(3, 3, B)
            srot, spos = np.array(cfg.sensor_rot[:]).reshape(3, 3), np.array(cfg.sensor_pos[:])
            o_s = xc + np.einsum("ijb,j->ib", Rc, spos)
            Rs = np.einsum("ijb,jk->ikb", Rc, srot)
            ms = -sum(_cross(f["x"][k] - o_s, f["F"][k]) for k in range(K))
            out["sensed"] = np.concatenate([np.einsum("jib,jb->ib", Rs, -Ft), np.einsum("jib,jb->ib", Rs, ms)])
        return out

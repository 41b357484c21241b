"""CPU reference of the external wrench on a link of the simulated plant (DESIGN "External wrench on a link"; numpy float64,
no GPU; test infrastructure). One substep is

    Oracle.set_state -> pose and Jacobian of the link from the oracle (a one-task oracle context whose MotionForceTask sits
    at the link origin: J, pos, R) -> tx = J_v^T F_w + J_w^T (M_w + (R c) x F_w) in numpy -> Oracle.sim_step(tau + tc + tx, h, 1)

and a period of s substeps is s such calls; tc is ContactReference.forces(q, dq)["tau"] when a contact is set. With joint
dynamics the step is JointDynamicsReference's, which takes tc + tx through its contact= hook (Combined below). The
countdown of `steps`, the status rows and the sensor rows are here too. The oracle is used through its existing entry
points only; the plant may be any object with set_state / get_state / sim_step over the batch (oracle_lib.Oracle, or
payload_cases.PayloadOracles for a plant whose robots carry payloads)."""
import numpy as np

import oracle_lib as ol

WORLD, LINK = 0, 1


def _cross(a, b):
    return np.cross(a, b, axis=0)


def active(steps):
    """steps > 0 or steps < 0 (a NaN: inactive)"""
    with np.errstate(invalid="ignore"):
        return (steps > 0) | (steps < 0)


def countdown(steps):
    """what a call of sai2b_sim_step leaves in the row: steps > 0 ? max(steps - 1, 0) : steps"""
    with np.errstate(invalid="ignore"):
        return np.where(steps > 0, np.maximum(steps - 1.0, 0.0), steps)


def sensor_rows(cfg, xc, Rc, x, Fw, Mw):
    """the reading of the ideal sensor of a MotionForceTask (cfg: its config, xc [3][B], Rc [9][B]: its control point and
    frame) of the wrench F_w, M_w ON the robot at x: o_s = x_c + R_c sensor_pos, R_s = R_c sensor_rot,
    f_s = R_s^T (-F_w), m_s = R_s^T (-(M_w + (x - o_s) x F_w)) -> [6][B]"""
    B = xc.shape[1]
    Rc = Rc.reshape(3, 3, B)
    srot, spos = np.array(cfg.sensor_rot[:]).reshape(3, 3), np.array(cfg.sensor_pos[:])
    o_s = xc + np.einsum("ijb,j->ib", Rc, spos)
    Rs = np.einsum("ijb,jk->ikb", Rc, srot)
    ms = -(Mw + _cross(x - o_s, Fw))
    return np.concatenate([np.einsum("jib,jb->ib", Rs, -Fw), np.einsum("jib,jb->ib", Rs, ms)])


class ExternalWrenchReference:
    def __init__(self, model, B, link, rows, point=(0.0, 0.0, 0.0), frame=WORLD, plant=None, contact=None, threads=8):
        """rows [7][B]: force 3, moment 3, steps; contact: a ContactReference (its forces(q, dq)["tau"] is tc)"""
        self.dof, self.B, self.link, self.frame = int(model.dof), B, int(link), int(frame)
        self.point = np.asarray(point, dtype=np.float64)
        self.rows = np.array(rows, dtype=np.float64)
        assert self.rows.shape == (7, B) and self.point.shape == (3,) and self.frame in (WORLD, LINK)
        at_origin = ol.motion_force_task("wrench_link", link=self.link, frame_pos=(0.0, 0.0, 0.0), robot_dof=self.dof)
        self.kin = ol.Oracle(model, [at_origin], B, threads=threads)
        self.plant = plant if plant is not None else ol.Oracle(model, [at_origin], B, threads=threads)
        self.contact = contact
        self.active = active(self.rows[6])  # of the call in progress, or of the last one

    # -- the law
    def wrench(self, q, dq):
        """-> dict x, Fw, Mw [3][B] (zeros for an inactive robot), tau [n][B] = tx, J [6][n][B], R [3][3][B]"""
        n, B = self.dof, self.B
        self.kin.set_state(np.ascontiguousarray(q), np.ascontiguousarray(dq))
        _, J, pos, rot = self.kin.get_model(0)
        J, R = J.reshape(6, n, B), rot.reshape(3, 3, B)
        r = np.einsum("ijb,j->ib", R, self.point)  # R c
        F, M = self.rows[0:3], self.rows[3:6]
        if self.frame == LINK:
            F, M = np.einsum("ijb,jb->ib", R, F), np.einsum("ijb,jb->ib", R, M)
        Fw, Mw = np.where(self.active, F, 0.0), np.where(self.active, M, 0.0)
        tx = np.einsum("inb,ib->nb", J[:3], Fw) + np.einsum("inb,ib->nb", J[3:], Mw + _cross(r, Fw))
        tx = np.where(self.active, tx, 0.0)
        return dict(x=pos + r, Fw=Fw, Mw=Mw, tau=tx, J=J, R=R)

    # -- the plant
    def set_state(self, q, dq):
        self.plant.set_state(np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(dq, dtype=np.float64))
        if self.contact is not None and self.contact.plant is not self.plant:
            self.contact.set_state(q, dq)

    def get_state(self):
        return self.plant.get_state()

    def begin(self):
        """entry of a call of sai2b_sim_step: who is pushed in it"""
        self.active = active(self.rows[6])

    def end(self):
        """exit of the call: the countdown"""
        self.rows[6] = countdown(self.rows[6])

    def step(self, tau, dt=0.001, substeps=1, with_gravity=False):
        """one control period of the plain step under the held torques tau [n][B] (None: zero)"""
        tau = np.zeros((self.dof, self.B)) if tau is None else np.asarray(tau, dtype=np.float64)
        h = dt / substeps
        self.begin()
        for _ in range(substeps):
            q, dq = self.plant.get_state()
            t = tau + self.contact.forces(q, dq)["tau"] if self.contact is not None else tau
            self.plant.sim_step(np.ascontiguousarray(t + self.wrench(q, dq)["tau"]), h, 1, bool(with_gravity))
        self.end()
        if self.contact is not None and self.contact.plant is not self.plant:
            self.contact.set_state(*self.plant.get_state())

    def joint_step(self, jd, tau, dt=0.001, substeps=1, with_gravity=False):
        """one control period of the step with joint dynamics: jd is a JointDynamicsReference made with contact=Combined(self)"""
        self.begin()
        jd.step(tau, dt, substeps, with_gravity)
        self.end()

    # -- what the kernel reports after the last substep
    def report(self, sensor=None, q=None, dq=None):
        """from the plant's current state (or q, dq) and the activity of the last call. sensor: None, or (oracle with the
        controller's hierarchy, task index) -> dict wrench_world [6][B], torque [n][B], robots_pushed, x [3][B], sensed [6][B]
        (None without a sensor)"""
        if q is None:
            q, dq = self.plant.get_state()
        w = self.wrench(q, dq)
        loaded = (self.rows[0:6] != 0).any(axis=0)
        out = dict(wrench_world=np.concatenate([w["Fw"], w["Mw"]]), torque=w["tau"], x=w["x"],
                   robots_pushed=int(np.count_nonzero(self.active & loaded)), sensed=None)
        if sensor is not None:
            o, task = sensor
            o.set_state(np.ascontiguousarray(q), np.ascontiguousarray(dq))
            _, _, xc, Rc = o.get_model(task)
            out["sensed"] = sensor_rows(o.tasks[task], xc, Rc, w["x"], w["Fw"], w["Mw"])
        return out


class Combined:
    """what JointDynamicsReference takes through its contact= hook: forces(q, dq)["tau"] = tc + tx"""

    def __init__(self, wrench):
        self.w = wrench

    def forces(self, q, dq):
        tx = self.w.wrench(q, dq)["tau"]
        return dict(tau=self.w.contact.forces(q, dq)["tau"] + tx if self.w.contact is not None else tx)

    def set_state(self, q, dq):
        if self.w.contact is not None:
            self.w.contact.set_state(q, dq)

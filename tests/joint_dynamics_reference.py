"""CPU reference of the joint dynamics of the simulated plant (DESIGN "Joint dynamics in the simulated plant"; numpy
float64, no GPU; test infrastructure). One substep is

    plant.set_state -> M from get_model(-1), b from get_bias -> the law below in numpy -> numpy.linalg.solve per robot
    -> plant.set_state of the result

and a period of s substeps is s such calls. The plant is oracle_lib.Oracle, or payload_cases.PayloadOracles for a plant
whose robots carry payloads; with a contact, ContactReference.forces supplies the contact torque tc. The oracle is used
through its existing entry points only.

    ts = min(max(tau, -t), t)
    sl = max(0, k max(0, lo - q) (1 - c dq))        su = max(0, k max(0, q - hi) (1 + c dq))
    g  = d + f / sqrt(dq^2 + e^2)
    (M + diag(a) + h diag(g)) dq+ = (M + diag(a)) dq + h (ts + sl - su + tc - b)         q+ = q + h dq+"""
import numpy as np

import oracle_lib as ol

ROWS = ("armature", "damping", "friction", "torque_limit", "q_lower", "q_upper")
NEUTRAL = dict(armature=0.0, damping=0.0, friction=0.0, torque_limit=np.inf, q_lower=-np.inf, q_upper=np.inf)


def saturate(tau, t):
    return np.minimum(np.maximum(tau, -t), t)


def stop_torques(q, dq, lo, hi, k, c):
    """-> sl, su (both >= 0): the lower stop pushes +, the upper one -"""
    sl = np.maximum(0.0, k * np.maximum(0.0, lo - q) * (1.0 - c * dq))
    su = np.maximum(0.0, k * np.maximum(0.0, q - hi) * (1.0 + c * dq))
    return sl, su


def dissipation(dq, d, f, e):
    """g of the law: the torque of damping and regularised Coulomb friction is -g dq"""
    return d + f / np.sqrt(dq * dq + e * e)


def rows_array(n, B, **rows):
    """[6][n][B] from scalars, [n] or [n][B] per name of ROWS (missing: neutral)"""
    out = np.empty((6, n, B))
    for r, name in enumerate(ROWS):
        v = rows.get(name)
        a = np.asarray(NEUTRAL[name] if v is None else v, dtype=np.float64)
        out[r] = a[:, None] if a.ndim == 1 else a
    return out


class JointDynamicsReference:
    def __init__(self, model, B, rows, stop_stiffness=0.0, stop_damping=0.0, friction_velocity_eps=1e-2, plant=None, contact=None,
                 threads=8):
        """rows [6][n][B] (ROWS); stop_stiffness, stop_damping, friction_velocity_eps: scalars or [n]; plant: an object with
        set_state / get_state / get_model(-1) / get_bias over the batch (default: an Oracle of `model`); contact: a
        ContactReference (its forces(q, dq)["tau"] is tc)"""
        self.n, self.B = int(model.dof), B
        n = self.n
        self.rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert self.rows.shape == (6, n, B)
        col = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)).copy()[:, None]
        self.k, self.c, self.e = col(stop_stiffness), col(stop_damping), col(friction_velocity_eps)
        self.plant = plant if plant is not None else ol.Oracle(model, [ol.joint_task("j", robot_dof=n)], B, threads=threads)
        self.contact = contact
        self.ts = np.zeros((n, B))
        self.saturated = np.zeros(B, dtype=bool)

    def set_state(self, q, dq):
        self.plant.set_state(np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(dq, dtype=np.float64))

    def get_state(self):
        return self.plant.get_state()

    def terms(self, q, dq, tau, with_gravity):
        """every piece of one substep at (q, dq) -> dict M [n][n][B], b, ts, sl, su, g, tc [n][B]"""
        n, B = self.n, self.B
        a, d, f, t, lo, hi = self.rows
        self.set_state(q, dq)
        M = np.asarray(self.plant.get_model(-1)).reshape(n, n, B)
        b = self.plant.get_bias(bool(with_gravity))
        sl, su = stop_torques(q, dq, lo, hi, self.k, self.c)
        tc = self.contact.forces(q, dq)["tau"] if self.contact is not None else np.zeros((n, B))
        return dict(M=M, b=b, ts=saturate(tau, t), sl=sl, su=su, g=dissipation(dq, d, f, self.e), tc=tc)

    def substep(self, q, dq, tau, h, with_gravity):
        """-> q+, dq+"""
        n = self.n
        a = self.rows[0]
        T = self.terms(q, dq, tau, with_gravity)
        Ma = T["M"] + np.eye(n)[:, :, None] * a[None]
        A = Ma + np.eye(n)[:, :, None] * (h * T["g"])[None]
        rhs = np.einsum("ijb,jb->ib", Ma, dq) + h * (T["ts"] + T["sl"] - T["su"] + T["tc"] - T["b"])
        dq1 = np.linalg.solve(A.transpose(2, 0, 1), rhs.T[:, :, None])[:, :, 0].T
        return q + h * dq1, np.ascontiguousarray(dq1)

    def step(self, tau, dt=0.001, substeps=1, with_gravity=False):
        """one control period under the held torques tau [n][B] (None: zero)"""
        tau = np.zeros((self.n, self.B)) if tau is None else np.asarray(tau, dtype=np.float64)
        h = dt / substeps
        q, dq = self.plant.get_state()
        for _ in range(substeps):
            q, dq = self.substep(q, dq, tau, h, with_gravity)
        self.set_state(q, dq)
        if self.contact is not None:
            self.contact.set_state(q, dq)
        t = self.rows[3]
        self.ts, self.saturated = saturate(tau, t), (np.abs(tau) > t).any(axis=0)

    def load(self, q, dq, tau):
        """the state and the held torques of a step made elsewhere, for report()"""
        self.set_state(q, dq)
        tau = np.zeros((self.n, self.B)) if tau is None else np.asarray(tau, dtype=np.float64)
        t = self.rows[3]
        self.ts, self.saturated = saturate(tau, t), (np.abs(tau) > t).any(axis=0)

    def report(self):
        """what the kernel reports after the last substep, from the plant's current state and the torques of the last step"""
        q, dq = self.plant.get_state()
        a, d, f, t, lo, hi = self.rows
        sl, su = stop_torques(q, dq, lo, hi, self.k, self.c)
        stop = sl - su
        return dict(applied_torque=self.ts, stop_torque=stop, dissipative_torque=-dissipation(dq, d, f, self.e) * dq,
                    robots_saturated=int(np.count_nonzero(self.saturated)), robots_at_stop=int(np.count_nonzero((stop != 0).any(axis=0))))

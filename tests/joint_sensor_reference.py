"""CPU reference of the joint sensors (include/sai2b.h "joint sensors"; numpy float64, no GPU; test infrastructure): one reading
as the law states it, vectorised over robots (or over unrelated records), and JointSensorReference, the per-robot state around
it: seeding, the sense stage, resets. The generator is the Philox / Box-Muller restatement of tests/hardware_reference.py.

One control period of a loop with a joint sensor is

    tau = controller.tick()            reads js.q_meas, js.dq_meas
    q, dq = plant.step(tau)            the truth
    js.step(q, dq, dt)                 the next reading
"""
import numpy as np

import hardware_reference as hr

STREAM = 10
MAX_DELAY = hr.MAX_DELAY
TACHOMETER, FINITE_DIFFERENCE = 0, 1
HALF_WINDOW = 1e-9  # records whose x / quantum lies this close to a half-integer are not compared: the tie could fall either way


def n_rows(dof):
    return 1 + 5 * dof


def ideal_rows(dof, B):
    rows = np.zeros((n_rows(dof), B))
    rows[1 + 4 * dof :] = 1.0
    return rows


def make_rows(dof, B, delay=0, offset=0.0, noise=0.0, quantum=0.0, velocity_noise=0.0, velocity_alpha=1.0):
    rows = np.empty((n_rows(dof), B))
    rows[0] = delay
    for k, a in enumerate((offset, noise, quantum, velocity_noise, velocity_alpha)):
        a = np.asarray(a, dtype=np.float64)
        rows[1 + k * dof : 1 + (k + 1) * dof] = a[:, None] if a.ndim == 1 and a.shape[0] == dof and dof != B else a
    return rows


def normals(m, e, robot, k0, k1, count):
    """m, e, robot, k0, k1 [K] -> z [count][K] of stream 10: call j gives z_4j .. z_4j+3"""
    out = []
    for j in range((count + 3) // 4):
        w = hr.philox4x32_10((m, e, np.full(np.shape(robot), 256 * STREAM + j), robot), (k0, k1))
        out += [*hr.box_muller(w[0], w[1]), *hr.box_muller(w[2], w[3])]
    return np.stack(out[:count])


def delay_of(rows, D):
    """the delay as the kernel reads it: (int) fmin(fmax(row 0, 0), D), a NaN gives 0"""
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(rows[0], 0.0), np.asarray(D, dtype=np.float64)).astype(np.int64)


def reading(rows, q, dq, dt, m, e, mode, D, robot, k0, k1, prev, filt, hist):
    """Reading m of episode e for K independent columns. rows [1 + 5 dof][K]; q, dq, prev, filt [dof][K]; dt, m, e, mode, D,
    robot, k0, k1 [K] (or scalars); hist [slots][2 dof][K] with slots > max D, written in place.
    -> dict p, v (the new pprev and filter state), q_meas, dq_meas, near_half [dof][K] (x / quantum within HALF_WINDOW of a tie)"""
    dof, K = q.shape
    m, e, mode, D, robot, k0, k1, dt = (np.broadcast_to(np.asarray(a), (K,)) for a in (m, e, mode, D, robot, k0, k1, dt))
    o, s, quantum, r, alpha = (rows[1 + k * dof : 1 + (k + 1) * dof] for k in range(5))
    z = normals(m, e, robot, k0, k1, 2 * dof)
    x = np.array(q, dtype=np.float64)
    x = np.where(o != 0.0, x + o, x)
    x = np.where(s != 0.0, x + s * z[:dof], x)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = x / quantum
        p = np.where(quantum > 0.0, quantum * np.rint(ratio), x)
        near_half = (quantum > 0.0) & (np.abs(np.abs(ratio - np.floor(ratio)) - 0.5) < HALF_WINDOW)
        fd = (p - prev) / dt
    base = np.where((mode == FINITE_DIFFERENCE) & (m > 0), fd, dq)
    w = np.where(r != 0.0, base + r * z[dof:], base)
    v = np.where((m == 0) | (alpha == 1.0), w, filt + alpha * (w - filt))
    cols = np.arange(K)
    d = delay_of(rows, D)
    past = np.maximum(m - d, 0)
    qm, dqm = p.copy(), v.copy()
    use = D > 0
    if use.any():
        c = cols[use]
        pv = np.concatenate([p, v])
        hist[(m % (D + 1))[use], :, c] = pv[:, use].T
        old = hist[(past % (D + 1))[use], :, c].T
        qm[:, use], dqm[:, use] = old[:dof], old[dof:]
    return dict(p=p, v=v, q_meas=qm, dq_meas=dqm, near_half=near_half)


class JointSensorReference:
    def __init__(self, dof, B, max_delay=0, rows=None, velocity_mode=TACHOMETER, seed=0, first_robot=0):
        self.dof, self.B, self.D, self.mode = dof, B, int(max_delay), int(velocity_mode)
        self.rows = ideal_rows(dof, B) if rows is None else np.array(rows, dtype=np.float64)
        assert self.rows.shape == (n_rows(dof), B) and 0 <= self.D <= MAX_DELAY and self.mode in (0, 1)
        self.k0, self.k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
        self.robot = first_robot + np.arange(B)
        self.c, self.e = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        self.prev, self.filt = np.zeros((dof, B)), np.zeros((dof, B))
        self.hist = np.zeros((self.D + 1, 2 * dof, B))
        self.q_meas, self.dq_meas = np.zeros((dof, B)), np.zeros((dof, B))
        self.near_half = np.zeros((dof, B), dtype=bool)

    def _take(self, q, dq, dt, m, mask):
        sel = np.flatnonzero(mask)
        hist = self.hist[:, :, sel]
        out = reading(self.rows[:, sel], np.asarray(q)[:, sel], np.asarray(dq)[:, sel], dt, m[sel], self.e[sel], self.mode, self.D, self.robot[sel],
                      self.k0, self.k1, self.prev[:, sel], self.filt[:, sel], hist)
        self.hist[:, :, sel] = hist
        self.prev[:, sel], self.filt[:, sel] = out["p"], out["v"]
        self.q_meas[:, sel], self.dq_meas[:, sel] = out["q_meas"], out["dq_meas"]
        self.near_half[:, sel] = out["near_half"]

    def seed(self, q, dq, mask=None, next_episode=False):
        """reading 0 of the selected robots (all: None), of their next episode when asked; their clock is left at 1"""
        mask = np.ones(self.B, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
        if next_episode:
            self.e = np.where(mask, self.e + 1, self.e)
        self._take(q, dq, 1.0, np.zeros(self.B, dtype=np.int64), mask)
        self.c = np.where(mask, 1, self.c)
        return self.q_meas.copy(), self.dq_meas.copy()

    def step(self, q, dq, dt):
        """the sense stage of one sai2b_sim_step: reading c of every robot; the clock is left at c + 1"""
        self._take(q, dq, dt, self.c.copy(), np.ones(self.B, dtype=bool))
        self.c = self.c + 1
        return self.q_meas.copy(), self.dq_meas.copy()

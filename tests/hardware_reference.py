"""CPU reference of the actuator and force-sensor models (include/sai2b.h "actuator and force-sensor models"; numpy float64,
no GPU; test infrastructure): Philox4x32-10 from its definition (vectorised, uint64 arithmetic), unit normals by Box-Muller,
the two stage laws and the reset bookkeeping. HardwareReference wraps any of the plant references (ExternalWrenchReference,
ContactReference, the joint-dynamics reference, a bare oracle): one control period is

    applied = hw.actuate(tau)
    the plant reference's step with `applied`
    sensed = hw.sense(the ideal sensor rows)        only when the plant wrote a reading in that call
    hw.advance()

or hw.period(tau, step, ideal) for the three in one."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
ACTUATOR, SENSOR = 0, 1
MAX_DELAY = 8


def philox4x32_10(counter, key):
    """counter [4][...], key [2][...] (anything that broadcasts), values in [0, 2^32) -> words [4][...] as uint64"""
    c = [np.asarray(x).astype(np.uint64) & MASK for x in counter]
    k = [np.asarray(x).astype(np.uint64) & MASK for x in key]
    shape = np.broadcast(*c, *k).shape
    c = [np.broadcast_to(x, shape).copy() for x in c]
    k = [np.broadcast_to(x, shape).copy() for x in k]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 bits: no overflow in 64
        c = [(p1 >> S32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> S32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return np.stack(c)


def box_muller(x0, x1):
    """two words -> two unit normals: u = (x + 0.5) 2^-32, r = sqrt(-2 ln u0), (r cos 2 pi u1, r sin 2 pi u1)"""
    u0, u1 = (x0.astype(np.float64) + 0.5) * 2.0**-32, (x1.astype(np.float64) + 0.5) * 2.0**-32
    r, a = np.sqrt(-2.0 * np.log(u0)), 6.283185307179586 * u1
    return r * np.cos(a), r * np.sin(a)


def normals(n, e, stream, robot, seed, count):
    """n, e, robot [B] -> z [count][B]: the first `count` normals of `stream` (call j gives z_4j .. z_4j+3)"""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = []
    for j in range((count + 3) // 4):
        w = philox4x32_10((n, e, np.full(np.shape(robot), 256 * stream + j), robot), key)
        out += [*box_muller(w[0], w[1]), *box_muller(w[2], w[3])]
    return np.stack(out[:count])


def ideal_rows(dof, B):
    """-> (actuator_rows [1 + 3 dof][B], sensor_rows [13][B]) of the ideal path"""
    act, sen = np.zeros((1 + 3 * dof, B)), np.zeros((13, B))
    act[1 : 1 + 2 * dof] = 1.0
    sen[12] = 1.0
    return act, sen


class HardwareReference:
    def __init__(self, dof, B, max_delay=0, actuator_rows=None, sensor_rows=None, seed=0, first_robot=0):
        ia, isen = ideal_rows(dof, B)
        self.dof, self.B, self.D, self.seed = dof, B, int(max_delay), int(seed)
        self.act = ia if actuator_rows is None else np.array(actuator_rows, dtype=np.float64)
        self.sen = isen if sensor_rows is None else np.array(sensor_rows, dtype=np.float64)
        assert self.act.shape == ia.shape and self.sen.shape == isen.shape and 0 <= self.D <= MAX_DELAY
        self.robot = first_robot + np.arange(B)
        self.n, self.e = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        self.hist = np.zeros((self.D + 1, dof, B))
        self.f, self.g, self.applied = np.zeros((dof, B)), np.zeros((6, B)), np.zeros((dof, B))

    def delay(self):
        """the delay as the kernel reads it: (int) fmin(fmax(row, 0), D), a NaN gives 0"""
        with np.errstate(invalid="ignore"):
            return np.fmin(np.fmax(self.act[0], 0.0), float(self.D)).astype(np.int64)

    def actuate(self, tau):
        """the commanded torques [dof][B] -> the applied ones"""
        dof, B, n = self.dof, self.B, self.n
        cols = np.arange(B)
        alpha, k, sigma = self.act[1 : 1 + dof], self.act[1 + dof : 1 + 2 * dof], self.act[1 + 2 * dof :]
        self.hist[n % (self.D + 1), :, cols] = np.asarray(tau, dtype=np.float64).T
        u = self.hist[np.maximum(n - self.delay(), 0) % (self.D + 1), :, cols].T
        self.f = np.where((n == 0) | (alpha == 1.0), u, self.f + alpha * (u - self.f))
        z = normals(n, self.e, ACTUATOR, self.robot, self.seed, dof)
        self.applied = k * self.f + sigma * z
        return self.applied.copy()

    def sense(self, ideal):
        """the ideal reading [6][B] as the plant left it -> the measured one"""
        z = normals(self.n, self.e, SENSOR, self.robot, self.seed, 6)
        y = (np.asarray(ideal, dtype=np.float64) + self.sen[0:6]) + self.sen[6:12] * z
        a = self.sen[12]
        self.g = np.where((self.n == 0) | (a == 1.0), y, self.g + a * (y - self.g))
        return self.g.copy()

    def advance(self):
        self.n = self.n + 1

    def period(self, tau, step, ideal=None):
        """one call of sai2b_sim_step: step(applied) runs the plant reference; ideal: None (no reading was written in this call),
        or a callable that gives the ideal rows [6][B] after the step -> (applied, sensed or None)"""
        applied = self.actuate(tau)
        step(applied)
        sensed = self.sense(ideal()) if ideal is not None else None
        self.advance()
        return applied, sensed

    def reset(self, mask):
        """sai2b_reset_robots: the selected robots start period 0 of their next episode; everything else is left (the law
        re-initialises the history and the filters at n = 0)"""
        m = np.asarray(mask).astype(bool)
        self.n = np.where(m, 0, self.n)
        self.e = np.where(m, self.e + 1, self.e)

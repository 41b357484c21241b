"""Poses of the robots of tests/robots.py spread over the singularity bands of a hierarchy's MotionForceTask (test
infrastructure, numpy only: the kinematics and the mass matrix come from the independent reading of the URDFs in
tests/urdf_np.py, nothing of the product's or the oracle's model code).

The SingularityHandler splits a task at the first singular value whose ratio to the largest is below s_max and blends
between s_min and s_max (SingularityHandler.cpp:100-121). For a task of rank r with ratios rho_i = s_i / s_0:
  regular  : rho_{r-1} >= s_max                       (no singular direction)
  blending : s_min < rho_{r-1} < s_max <= rho_{r-2}   (one direction, 0 < alpha < 1)
  inside   : rho_{r-1} < s_min, rho_{r-2} >= s_max    (one direction, alpha = 0)
  two      : rho_{r-2} < s_max                         (two directions at once)
A pose of a singular band is found on the segment between a singular pose of the robot's own families (planar_4r:
links stretched or folded back; six_r: elbow straight, wrist aligned, wrist centre over the shoulder axis;
sliding_base: the Panda rules of workloads.sample_poses, elbow near its limit, q6 near 0, slider anywhere) and a
regular pose, by bisection on rho to a ratio drawn inside the band, away from its edges by MARGIN."""
import functools

import numpy as np

import robots
import urdf_np

S_MIN, S_MAX = 6e-3, 6e-2  # the task defaults (SingularityHandler.cpp:10-20), what every hierarchy of the tests runs with
MARGIN = 1.25  # a band's ratios stay this factor inside its edges: the oracle's SVD and ours agree far beyond that
BANDS = ("regular", "blending", "inside", "two")

# per hierarchy (named as in test_gpu_robot_routes): robot, the MotionForceTask's link and point, its rows of the 6 x n
# Jacobian, the joints a JointTask above it selects (its dynamically consistent nullspace projects the task's Jacobian)
# and the bands the task's geometry can reach
TASKS = {
    "planar_4r": dict(robot="planar_4r", link="link4", point=(0.5, 0.0, 0.0), rows=[0, 1, 5], above=None,
                      # (three rows, four parallel axes: rank 1 would need every joint at one point — one direction at most)
                      bands=("regular", "blending", "inside")),
    # (a position task on six joints: the wrist's offsets keep a second direction out of reach in practice)
    "six_r": dict(robot="six_r", link="link6", point=(0.05, 0.0, 0.02), rows=[0, 1, 2], above=None,
                  bands=("regular", "blending", "inside")),
    "six_r_mft6": dict(robot="six_r", link="link6", point=(0.05, 0.0, 0.02), rows=list(range(6)), above=None, bands=BANDS),
    "sliding_base": dict(robot="sliding_base", link="end-effector", point=(0.0, 0.0, 0.07), rows=list(range(6)), above=[0, 7],
                         bands=BANDS),
}


@functools.lru_cache(maxsize=None)
def chain(robot):
    return urdf_np.Chain(robots.TEXT[robot](), is_file=False)


def limits(robot):
    import sai2_primitives_perso_amd as pkg

    m, _ = pkg.model_from_urdf(robots.TEXT[robot](), is_file=False)
    n = m.dof
    return np.array(list(m.q_lower)[:n]), np.array(list(m.q_upper)[:n])


def task_jacobian(name, q):
    """the rows of the task's Jacobian the SingularityHandler decomposes: J N_prec (N_prec = I - Jbar S of the JointTask
    above, dynamically consistent)"""
    t = TASKS[name]
    ch = chain(t["robot"])
    J, _, _ = ch.jacobian(q, t["link"], t["point"])
    J = J[t["rows"]]
    if t["above"] is not None:
        M, _ = ch.mass_matrix_and_gravity(q)
        S = np.zeros((len(t["above"]), ch.dof))
        S[np.arange(len(t["above"])), t["above"]] = 1
        Minv = np.linalg.inv(M)
        Jbar = Minv @ S.T @ np.linalg.inv(S @ Minv @ S.T)
        J = J @ (np.eye(ch.dof) - Jbar @ S)
    return J


def ratios(name, q):
    s = np.linalg.svd(task_jacobian(name, q), compute_uv=False)
    return s / s[0]


def band_of(name, q):
    r = len(TASKS[name]["rows"])
    rho = ratios(name, q)
    if rho[r - 2] < S_MAX:
        return "two"
    if rho[r - 1] >= S_MAX:
        return "regular"
    return "blending" if rho[r - 1] > S_MIN else "inside"


def _newton_to_zero(name, q, idx, lo, hi, frozen=(), iters=25):
    """drive rho_idx to zero (a singular pose) by Newton steps on the singular value, numerical gradient; None if it
    does not get there inside the joint limits"""
    q = q.copy()
    for _ in range(iters):
        f = ratios(name, q)[idx]
        if f < 1e-9:
            return q
        g = np.zeros_like(q)
        for j in range(q.size):
            if j in frozen:
                continue
            d = np.zeros_like(q)
            d[j] = 1e-6
            g[j] = (ratios(name, q + d)[idx] - f) / 1e-6
        if not np.any(g):
            return None
        q = np.clip(q - f * g / (g @ g), lo, hi)
    return q if ratios(name, q)[idx] < 1e-6 else None


def _seed(name, rng, lo, hi, two):
    """a singular pose of one of the robot's families (two: with two singular directions)"""
    t = TASKS[name]
    r = len(t["rows"])
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    q = mid + 0.6 * half * rng.uniform(-1, 1, lo.size)
    fam = rng.integers(2)
    if t["robot"] == "planar_4r":
        if fam == 0:  # stretched: exactly singular
            q[1:] = 0
        else:  # folded back at the joint limits (ratio ~0.05: the blending band only)
            q[1:] = np.array([1, -1, 1]) * rng.choice([-1, 1]) * (hi[1:] - rng.uniform(0, 0.02, 3))
        return q
    if t["robot"] == "six_r":
        q[4] = 0.0  # wrist straight (axes 4 and 6 aligned)
        if r == 6 and not two and fam == 0:
            return q
        if fam == 0:
            q[2] = 2.7  # elbow close to straight
        else:
            q[1] = -0.3  # wrist centre near the shoulder axis
        frozen = (4,) if (r == 6 and two) else ()
        q = _newton_to_zero(name, q, r - 1, lo, hi, frozen)
        if q is not None and two:
            q = _newton_to_zero(name, q, r - 2, lo, hi, frozen)
        return q
    # sliding_base: the Panda rules, slider anywhere
    q[0] = rng.uniform(lo[0], hi[0])
    q[6] = 0.0
    if two or fam == 0:
        q[4] = hi[4] - rng.uniform(0, 0.01)
    return q


def _bisect(name, q_s, q_r, idx, target, iters=40):
    a, b = 0.0, 1.0  # rho(q_s) < target <= rho(q_r)
    for _ in range(iters):
        m = 0.5 * (a + b)
        if ratios(name, q_s + m * (q_r - q_s))[idx] < target:
            a = m
        else:
            b = m
    return q_s + b * (q_r - q_s)


def _target(rng, band):
    lo, hi = {"blending": (S_MIN * MARGIN, S_MAX / MARGIN), "inside": (S_MIN / 30, S_MIN / MARGIN),
              "two": (S_MIN / 10, S_MAX / MARGIN)}[band]
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def _clear_of_edges(name, q, band):
    """the pose's band does not depend on rounding: every ratio that decides it is MARGIN away from s_min and s_max"""
    r = len(TASKS[name]["rows"])
    rho = ratios(name, q)
    for k in (r - 2, r - 1):
        for e in (S_MIN, S_MAX):
            if e / MARGIN < rho[k] < e * MARGIN:
                return False
    return band_of(name, q) == band


@functools.lru_cache(maxsize=None)
def _pool(name, band, n, seed):
    t = TASKS[name]
    lo, hi = limits(t["robot"])
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rng = np.random.default_rng([seed, BANDS.index(band), len(name)])
    r = len(t["rows"])
    out = []
    for _ in range(200 * n):
        if len(out) == n:
            break
        q_r = mid + 0.6 * half * rng.uniform(-1, 1, lo.size)
        if band == "regular":
            if _clear_of_edges(name, q_r, band):
                out.append(q_r)
            continue
        q_s = _seed(name, rng, lo, hi, band == "two")
        if q_s is None or band_of(name, q_r) != "regular":
            continue
        idx = r - 2 if band == "two" else r - 1
        target = _target(rng, band)
        if ratios(name, q_s)[idx] >= target:
            continue
        q = _bisect(name, q_s, q_r, idx, target)
        if _clear_of_edges(name, q, band):
            out.append(q)
    assert len(out) == n, (name, band, len(out))
    return np.array(out).T.copy()


def poses(name, band, n, seed=0):
    """q [dof][n] of the band (C-contiguous; deterministic in the arguments)"""
    return _pool(name, band, n, seed).copy()


def mixed(name, B, seed=0, per_band=16):
    """B poses, the task's bands in turn (robot b is of band (b + 1) % len(bands)): a pool of per_band poses per band, repeated
    for larger batches. Returns q [dof][B] and the band index of every robot."""
    bands = TASKS[name]["bands"]
    pools = [poses(name, b, per_band, seed) for b in bands]
    k = np.arange(B)
    which = (k + 1) % len(bands)  # (a one-robot batch is in the blending band)
    q = np.empty((pools[0].shape[0], B))
    for i in range(len(bands)):
        sel = which == i
        q[:, sel] = pools[i][:, (k[sel] // len(bands)) % per_band]
    return q, np.array([BANDS.index(bands[i]) for i in which])

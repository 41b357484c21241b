"""Inputs of the whole-arm contact tests (tests/test_body_contact_reference.py on the CPU, tests/test_gpu_body_contact.py on the
GPU), drawn with fixed seeds. One table, so that the CPU file checks the conditioning of exactly what the GPU file runs.

A cell is (robot, B, categories, dissipative): planar_4r, six_r, the Panda and sliding_base (prismatic joint 0; 4, 6, 7 and 8
joints) at B = 1, 63, 64, 65, 200 and the Panda at 4 099; plane alone, obstacle alone, self alone, all three; with and without
friction and damping. The eight combinations are dealt over the 20 (robot, B) cells (COMBOS), each occurs at least twice.

The inputs are built PER ROBOT, relative to that robot's own sphere centres (geometry 'arm' of tests/collision_cases.py, 12 spheres):
  robot b with b % 3 == 0 is DESIGNATED: two candidates of the cell's categories penetrate by 1 to 20 mm at the start. Planes: two
      planes, each put under the sphere that is lowest along its normal. Obstacles: two obstacles, each pushed into a sphere of its
      own from a direction in which it reaches no other sphere by more than 20 mm. Self: the robot's q is taken from a pool of
      drawn postures whose deepest pair penetrates by 1 to 20 mm (two pairs where the pool has such a posture).
  robot b with b % 3 == 1 NEVER touches: its planes and obstacles are absent (NaN) or 0.5 m away, its q comes from the pool of
      postures whose pairs all clear by more than 40 mm.
  robot b with b % 3 == 2 is a near miss (1 to 5 mm of clearance and an approach velocity) or, every other one, designated too.
So at least a quarter of the robots (a half of them, and the single robot of B = 1) have f_n > 0 in some substep, at least a
tenth (a third, rounded down) never touch, and at least one has two candidates active at once:
tests/test_body_contact_reference.py asserts all three from the reference for every cell, and that the state stays finite and
every penetration stays below the sphere's radius over the whole run.

Stiffness 1e4 to 3e4 N/m; h = dt / 3 = 3.3e-4 s; the lightest effective mass at a sphere is about 0.5 kg for the Panda, so
h sqrt(k / m_eff) is about 0.07: far below 1, the explicit spring is stable. Damping 0 to 0.3 s/m, friction 0 to 0.8."""
import zlib

import numpy as np

import collision_cases as cc
import sai2_primitives_perso_amd as pkg
from body_contact_reference import ALL, OBSTACLE, PLANE, SELF, BodyContactReference
from collision_reference import CollisionReference, product_spheres

PERIODS, SUBSTEPS, DT = 5, 3, 1e-3
# per robot, the combination of every batch size. Self alone stands with six_r and sliding_base: of 30 000 drawn postures these two
# have some with two pairs in touch at once, planar_4r (5 pairs) and the Panda have none, and every cell must hold a robot with
# two candidates active at once; their self pairs push in the cells with all three categories.
D, E = True, False
COMBOS = dict(planar_4r=((PLANE, D), (OBSTACLE, D), (ALL, D), (PLANE, E), (ALL, E)),
              six_r=((SELF, D), (OBSTACLE, E), (PLANE, D), (ALL, E), (SELF, E)),
              panda=((ALL, D), (PLANE, E), (OBSTACLE, D), (ALL, E), (OBSTACLE, E)),
              sliding_base=((SELF, E), (ALL, D), (PLANE, E), (SELF, D), (OBSTACLE, D)))
V_EPS = 1e-3


def _cells():
    out = []
    for ri, robot in enumerate(cc.ROBOTS):
        for bi, B in enumerate(cc.BATCHES):
            cats, dis = COMBOS[robot][bi]
            out.append((robot, B, cats, dis))
    out.append(("panda", 4099, ALL, True))
    return tuple(out)


CELLS = _cells()
TWIN_CELL = ("panda", 130, ALL, True)
FORMS_CELL = ("panda", 200, ALL, True)
MOVE_CELL = ("six_r", 65, OBSTACLE, True)
DEVICE_ROWS_CELL = ("sliding_base", 65, ALL, True)
LOOP_CELL = ("panda", 200, ALL, True)
FACADE_CELL = ("panda", 64, ALL, True)
DRAWN_CELLS = CELLS + (TWIN_CELL, MOVE_CELL, DEVICE_ROWS_CELL)


def cell_id(c):
    return f"{c[0]}-{c[1]}-{''.join(n for n, b in (('plane', PLANE), ('obstacle', OBSTACLE), ('self', SELF)) if c[2] & b)}-{'dissipative' if c[3] else 'elastic'}"


_pools = {}
PAIR_GAP, FREE = 3, 40e-3


def pairs(robot):
    """the tested pairs [(i, j)]: spheres whose links are at least PAIR_GAP apart (the default of 2 would pair the Panda's links 4
    and 6, whose spheres overlap in every posture: joint 7 stands 88 mm from joint 6)"""
    links = CollisionReference(cc.model(robot)[2], cc.geometry(robot, "arm")).links
    return [(i, j) for i in range(len(links)) for j in range(i + 1, len(links)) if abs(links[i] - links[j]) >= PAIR_GAP]


def pair_mask(robot):
    pm = [0] * 16
    for i, j in pairs(robot):
        pm[i] |= 1 << j
    return pm



def _pool(robot):
    """postures of `robot` sorted by what its default pairs do: 'touch' (deepest pair 1..20 mm in), 'double' (two pairs 1..20 mm in),
    'free' (every pair clears by > FREE); each an array [n][K]"""
    if robot not in _pools:
        m, links, text = cc.model(robot)
        n = int(m.dof)
        spheres = cc.geometry(robot, "arm")
        col = CollisionReference(text, spheres, pair_mask=pair_mask(robot))
        ref = BodyContactReference(col, m, 1, np.zeros((3, 1)), plant=object())
        rng = np.random.default_rng([zlib.crc32(robot.encode()), 77])
        lo, hi = np.array(m.q_lower[:n]), np.array(m.q_upper[:n])
        K = 30000
        q = (lo + (hi - lo) * rng.uniform(0.1, 0.9, (K, n))).T
        x = ref.kinematics(q)[0]
        r = [s[2] for s in spheres]
        pen = np.array([r[i] + r[j] - np.linalg.norm(x[i] - x[j], axis=1) for i in range(len(r)) for j in range(i + 1, len(r)) if (col.pair_mask[i] >> j) & 1])
        deepest = pen.max(axis=0)
        inside = ((pen > 1e-3) & (pen < 20e-3)).sum(axis=0)
        touch = (deepest > 1e-3) & (deepest < 20e-3)
        _pools[robot] = dict(touch=q[:, touch & (inside == 1)], double=q[:, touch & (inside >= 2)], free=q[:, deepest < -FREE])
        assert _pools[robot]["free"].shape[1] >= 64 and _pools[robot]["touch"].shape[1] + _pools[robot]["double"].shape[1] >= 16, \
            (robot, {k: v.shape for k, v in _pools[robot].items()})
    return _pools[robot]


def designation(B):
    """per robot: 2 designated, 0 never touches, 1 near miss"""
    b = np.arange(B)
    return np.where(b % 3 == 0, 2, np.where(b % 3 == 1, 0, np.where(b % 6 == 2, 2, 1)))


def draw(cell, state=None):
    """state: (q, dq, tau) [n][B] to build the environment around instead of the drawn ones (the self pairs then touch by chance
    alone) -> dict: model, reference (BodyContactReference on a CollisionReference), idx / cen / rad (the product's spheres), q, dq, tau
    [n][B], env [28][B] (2 planes, 4 obstacles... the cell's P and O), rows [3][B], P, O, n, B, categories, role [B]"""
    robot, B, cats, dissipative = cell
    m, links, text = cc.model(robot)
    n = int(m.dof)
    rng = np.random.default_rng([zlib.crc32(robot.encode()), B, cats, int(dissipative), 20261021])
    spheres = cc.geometry(robot, "arm")
    P, O = 2, 2
    col = CollisionReference(text, spheres, P, O, pair_mask=pair_mask(robot))
    idx, cen, rad = product_spheres(pkg, links, spheres)
    role = designation(B)
    pool = _pool(robot)
    q = np.empty((n, B))
    for b in range(B):
        if (cats & SELF) and role[b] == 2:
            src = pool["double"] if (pool["double"].shape[1] and (b == 0 or rng.random() < 0.3)) or not pool["touch"].shape[1] else pool["touch"]
        else:
            src = pool["free"]
        q[:, b] = src[:, rng.integers(src.shape[1])]
    dq = rng.uniform(-0.5, 0.5, (n, B))
    tau = rng.uniform(-2.0, 2.0, (n, B))
    if state is not None:
        q, dq, tau = (np.array(a, dtype=np.float64) for a in state)
    rows = np.stack([rng.uniform(1e4, 3e4, B), rng.uniform(0.0, 0.3, B) if dissipative else np.zeros(B),
                     rng.uniform(0.0, 0.8, B) if dissipative else np.zeros(B)])
    ref = BodyContactReference(col, m, B, rows, categories=cats, v_eps=V_EPS)
    x = ref.kinematics(q)[0].transpose(1, 0, 2)  # [B][S][3]
    r = np.array([s[2] for s in spheres])
    S = len(r)
    env = np.full((6 * P + 4 * O, B), np.nan)
    for b in range(B):
        if role[b] == 0:
            if b % 2:  # present, and far away
                for p in range(P):
                    nrm = rng.normal(size=3)
                    nrm /= np.linalg.norm(nrm)
                    env[6 * p + 3 : 6 * p + 6, b] = nrm
                    env[6 * p : 6 * p + 3, b] = nrm * ((nrm @ x[b].T - r).min() - 0.5)
                for o in range(O):
                    u = rng.normal(size=3)
                    env[6 * P + 4 * o : 6 * P + 4 * o + 3, b] = x[b].mean(axis=0) + 3.0 * u / np.linalg.norm(u)
                    env[6 * P + 4 * o + 3, b] = 0.05
            continue
        gap = (lambda: -rng.uniform(1e-3, 20e-3)) if role[b] == 2 else (lambda: rng.uniform(1e-3, 5e-3))  # clearance, < 0: penetration
        for p in range(P):
            nrm = rng.normal(size=3)
            nrm /= np.linalg.norm(nrm)
            s = nrm @ x[b].T - r  # the lowest point of every sphere along the normal
            env[6 * p + 3 : 6 * p + 6, b] = nrm
            env[6 * p : 6 * p + 3, b] = nrm * (s.min() - gap()) + rng.normal(size=3) @ (np.eye(3) - np.outer(nrm, nrm))
        for o in range(O):
            ro = rng.uniform(0.03, 0.06)
            for _ in range(200):  # a direction from which the obstacle reaches its own sphere alone (others by at most 20 mm)
                k = int(rng.integers(S))
                u = rng.normal(size=3)
                u /= np.linalg.norm(u)
                g = gap()
                c = x[b, k] + u * (r[k] + ro + g)
                pen = r + ro - np.linalg.norm(x[b] - c, axis=1)
                pen[k] = -1.0
                if pen.max() < min(20e-3, -g if g < 0 else 0.0):
                    break
            else:
                raise AssertionError(("no free direction for an obstacle", cell, b))
            env[6 * P + 4 * o : 6 * P + 4 * o + 3, b], env[6 * P + 4 * o + 3, b] = c, ro
    ref.env = env
    return dict(model=m, links=links, spheres=spheres, reference=ref, collision=col, idx=idx, cen=cen, rad=rad, q=q, dq=dq, tau=tau, env=env,
                rows=rows, P=P, O=O, n=n, B=B, categories=cats, role=role, text=text)


_ran = {}


def ran(cell):
    """(case, run) of a cell, computed once and shared: run = dict q, dq [PERIODS][n][B], status [PERIODS][9 + n][B], counts
    [PERIODS][4], substeps: forces() of every substep (PERIODS * SUBSTEPS), reports: forces() at every period's end"""
    if cell not in _ran:
        case = draw(cell)
        ref = case["reference"]
        ref.set_state(case["q"], case["dq"])
        run = dict(q=[], dq=[], status=[], counts=[], substeps=[], reports=[])
        for _ in range(PERIODS):
            ref.step(case["tau"], DT, SUBSTEPS, watch=run["substeps"])
            qq, dd = ref.get_state()
            rep = ref.report()
            run["q"].append(np.array(qq)), run["dq"].append(np.array(dd))
            run["status"].append(rep["status"]), run["counts"].append(rep["counts"]), run["reports"].append(rep["forces"])
        _ran[cell] = (case, run)
    return _ran[cell]


def category_names(cats):
    return tuple(name for name, bit in (("plane", PLANE), ("obstacle", OBSTACLE), ("self", SELF)) if cats & bit)

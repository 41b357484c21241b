"""Inputs of the collision tests (tests/test_collision_reference.py on the CPU, tests/test_gpu_collision.py on the GPU): robots,
sphere geometries, joint positions, planes and obstacles, all drawn with fixed seeds. One table, so that the CPU file checks the
conditioning (well-separated minima, margins and normalised distances) of exactly what the GPU file runs.

Geometries: 'last' one sphere on the last link; 'arm' one sphere per moving link and further ones on alternate links up to 12;
'full16' sixteen spheres over the world (link -1), inner links and the last link. A sphere is (URDF link name | None, centre in
that link, radius), as tests/collision_reference.py takes it."""
import zlib

import numpy as np

import hp_fixture
import sai2_primitives_perso_amd as pkg
from collision_reference import CollisionReference, product_spheres

ROBOTS = ("planar_4r", "six_r", "panda", "sliding_base")
BATCHES = (1, 63, 64, 65, 200)
MARGINS = (0.25, 0.3, 0.05)
PITCHED_BASE = (np.array([0.1, -0.2, 0.3]), np.array([[np.cos(0.4), 0, np.sin(0.4)], [0, 1, 0], [-np.sin(0.4), 0, np.cos(0.4)]]))

_models = {}


def model(robot):
    """(RobotModel, UrdfLinks, URDF text) of a robot, loaded once"""
    if robot not in _models:
        text = hp_fixture.urdf_text(robot)
        m, links = pkg.model_from_urdf(text, is_file=False)
        _models[robot] = (m, links, text)
    return _models[robot]


def moving_links(robot):
    import urdf_np

    return [j["child"] for j in urdf_np.Chain(model(robot)[2], is_file=False).moving]


def geometry(robot, kind):
    names = moving_links(robot)
    n = len(names)
    rng = np.random.default_rng([zlib.crc32(robot.encode()), zlib.crc32(kind.encode())])
    c = lambda: rng.uniform(-0.06, 0.06, 3)
    r = lambda: float(rng.uniform(0.03, 0.07))
    if kind == "last":
        return [(names[-1], c(), r())]
    if kind == "arm":
        sph = [(nm, c(), r()) for nm in names]
        k = 0
        while len(sph) < 12:
            sph.append((names[k % n], c() + [0.0, 0.0, 0.1], r()))
            k += 2
        return sph
    if kind == "full16":
        sph = [(None, rng.uniform(-0.5, 0.5, 3), r()) for _ in range(3)]
        sph += [(names[-1], c(), r()) for _ in range(2)]
        k = 0
        while len(sph) < 16:
            sph.append((names[k % n], c() + [0.0, 0.05 * (k // n), 0.0], r()))
            k += 1
        return sph
    raise KeyError(kind)


# (robot, B, geometry, planes, obstacles, pairs, pitched base, NaN plane on every third robot, NaN in q of some robots)
def _cells():
    geoms = ("arm", "last", "full16", "arm", "full16")
    planes = (1, 2, 0, 2, 1)
    obstacles = (1, 0, 4, 4, 1)
    pairs = ("default", "none", "all", "default", "all")
    out = []
    for ri, robot in enumerate(ROBOTS):
        for bi, B in enumerate(BATCHES):
            k = (bi + ri) % 5
            out.append((robot, B, geoms[k], planes[k], obstacles[k], pairs[k], k == 2 or (ri == 1 and bi == 0), planes[k] > 0 and bi % 2 == 1, bi == 4))
    out.append(("panda", 4099, "arm", 1, 2, "default", False, True, True))
    return tuple(out)


CELLS = _cells()
# the cells of the other GPU tests: block subsets, view, the twin run, rows rewritten on the device, shards, argument checks, the
# resident loop of tests/test_gpu_end_episodes.py
SUBSET_CELL = ("panda", 65, "arm", 1, 1, "default", False, False, False)
VIEW_CELL = ("six_r", 65, "arm", 1, 1, "default", False, False, False)
TWIN_CELL = ("panda", 130, "arm", 1, 2, "default", False, False, False)
TORCH_CELL = ("sliding_base", 65, "arm", 1, 2, "default", False, False, False)
SHARD_CELL = ("panda", 200, "arm", 2, 1, "default", False, True, True)
ARG_CELL = ("panda", 63, "arm", 2, 4, "default", False, False, False)
LOOP_CELL = ("panda", 200, "arm", 1, 2, "default", False, False, False)
DRAWN_CELLS = CELLS + (SUBSET_CELL, VIEW_CELL, TWIN_CELL, TORCH_CELL, SHARD_CELL, ARG_CELL, LOOP_CELL)


def pair_mask(pairs, links):
    n = len(links)
    if pairs == "none":
        return [0] * 16
    if pairs == "all":
        return [(((1 << n) - 1) & ~((2 << i) - 1)) if i < n else 0 for i in range(16)]
    return None  # the default


def draw(cell, seed=0):
    """-> dict: model, links, spheres, reference (CollisionReference), idx / cen / rad (the product's spheres), q [n][B], env
    [6 P + 4 O][B] or None, pair_mask (None: the default), base"""
    robot, B, geom, P, O, pairs, pitched, nan_plane, nan_q = cell
    m, links, text = model(robot)
    n = int(m.dof)
    rng = np.random.default_rng([zlib.crc32(robot.encode()), B, zlib.crc32(geom.encode()), P, O, seed])
    lo, hi = np.array(m.q_lower[:n]), np.array(m.q_upper[:n])
    q = np.ascontiguousarray((lo + (hi - lo) * rng.uniform(0.2, 0.8, (B, n))).T)
    spheres = geometry(robot, geom)
    base = PITCHED_BASE if pitched else None
    idx, cen, rad = product_spheres(pkg, links, spheres)
    pm = pair_mask(pairs, idx)
    ref = CollisionReference(text, spheres, P, O, pair_mask=pm, margins=MARGINS, base=base)
    env = None
    if P + O:
        env = np.empty((6 * P + 4 * O, B))
        for p in range(P):
            nrm = rng.normal(size=(3, B))
            nrm /= np.linalg.norm(nrm, axis=0)
            env[6 * p + 3 : 6 * p + 6] = nrm
            env[6 * p : 6 * p + 3] = rng.uniform(-0.3, 0.3, (3, B)) - nrm * rng.uniform(0.2, 0.9, B)
        for o in range(O):
            env[6 * P + 4 * o : 6 * P + 4 * o + 3] = rng.uniform(-0.9, 0.9, (3, B))
            env[6 * P + 4 * o + 3] = rng.uniform(0.05, 0.15, B)
        if nan_plane:
            env[rng.integers(0, 6), ::3] = np.nan
    if nan_q:
        q[0, 7::50] = np.nan
        q[n - 1, 11::50] = np.inf
    mdl = m if base is None else pkg.with_base_transform(m, base[0], base[1])
    return dict(model=mdl, links=links, spheres=spheres, reference=ref, idx=idx, cen=cen, rad=rad, q=q, env=env, pair_mask=pm, base=base,
                P=P, O=O, n=n, B=B)


_evaluated = {}


def evaluated(cell):
    """(case, reference outputs) of a cell, computed once and shared"""
    if cell not in _evaluated:
        case = draw(cell)
        _evaluated[cell] = (case, case["reference"].evaluate(case["q"], case["env"]))
    return _evaluated[cell]

"""CPU tests of tests/collision_reference.py, the numpy restatement the collision kernel and the law's header are held to: known
answers computed by hand (which pins the specification itself), the gradient against a central difference of the distance on the
40-digit kinematics of tests/hp_reference.Model, the tie rule, the empty category and the NaN plane, and the conditioning of every
input cell the GPU tests draw.

Central difference: D(q) is the winner's distance evaluated with mpmath at 40 digits, step h = 1e-10: truncation h^2 |D'''| / 6 ~
1e-20, rounding 1e-40 / h = 1e-30. What is left is the float64 rounding of the reference's own gradient, a sum of dof products
of O(1) numbers: 1e-15. Bound 1e-12, the project's bound for pose rows."""
import numpy as np
import pytest
from mpmath import mp, mpf

import collision_cases as cc
import hp_reference as hp
import robots
from collision_reference import CollisionReference, default_masks

PLANAR = robots.planar_4r_urdf()


def _env(planes=(), obstacles=()):
    return np.array([v for p0, n in planes for v in (*p0, *n)] + [v for c, r in obstacles for v in (*c, r)], dtype=float)


# ---------------------------------------------------------------------------------------------- known answers
def test_a_sphere_over_a_plane():
    """planar_4r stretched along x: link4's frame sits at (1.5, 0, 0); a sphere of radius 0.1 at (0.25, 0, 0) in it is at
    (1.75, 0, 0). Plane through (0, -0.5, 0) with normal +y: d = 0.5 - 0.1. Every joint turns about z through (0 | 0.5 | 1 | 1.5, 0,
    0): dx/dq_m = z x (x - o_m) = (0, 1.75 - o_m, 0), so g = (1.75, 1.25, 0.75, 0.25)."""
    ref = CollisionReference(PLANAR, [("link4", (0.25, 0, 0), 0.1)], n_planes=1, margins=(0.41, 0, 0))
    r = ref.one(np.zeros(4), _env(planes=[((0, -0.5, 0), (0, 1, 0))]))
    p = r["plane"]
    assert abs(p["distance"] - 0.4) < 1e-15 and p["index"] == 0 and np.array_equal(p["normal"], [0, 1, 0])
    assert np.abs(p["gradient"] - [1.75, 1.25, 0.75, 0.25]).max() < 1e-15
    assert np.abs(r["centres"][0] - [1.75, 0, 0]).max() < 1e-15 and r["flags"] == 1
    assert r["obstacle"]["distance"] == np.inf and r["self"]["index"] == -1
    # the margin is strict
    assert CollisionReference(PLANAR, [("link4", (0.25, 0, 0), 0.1)], n_planes=1, margins=(p["distance"], 0, 0)).one(
        np.zeros(4), _env(planes=[((0, -0.5, 0), (0, 1, 0))]))["flags"] == 0


def test_two_spheres():
    """q = (0, pi/2, 0, 0): sphere A at joint 0's origin on link1, sphere B at link4's origin (0.5, 1, 0). |xA - xB| = sqrt(1.25),
    u = (-0.5, -1, 0) / sqrt(1.25). A does not move; dxB/dq = z x (xB - o_m) with o = (0,0,0), (0.5,0,0), (0.5,0.5,0), (0.5,1,0):
    g = -u . dxB/dq = (0, -0.5, -0.25, 0) / sqrt(1.25)."""
    ref = CollisionReference(PLANAR, [("link1", (0, 0, 0), 0.05), ("link4", (0, 0, 0), 0.07)], margins=(0, 0, 1.0))
    assert ref.links == [0, 3] and ref.pair_mask[0] == 2 and ref.env_mask == 3
    r = ref.one(np.array([0, np.pi / 2, 0, 0]), _env())
    s, L = r["self"], np.sqrt(1.25)
    assert abs(s["distance"] - (L - 0.12)) < 1e-15 and s["index"] == 1 and abs(s["norm"] - L) < 1e-15
    assert np.abs(s["normal"] - np.array([-0.5, -1, 0]) / L).max() < 1e-15
    assert np.abs(s["gradient"] - np.array([0, -0.5, -0.25, 0]) / L).max() < 1e-15
    assert r["flags"] == 4


def test_a_world_sphere_under_a_rotated_base():
    """the base at (1, 0, 0), turned a quarter about z: link4's origin (1.5, 0, 0) in the base is (1, 1.5, 0) in the world. A sphere
    on link -1 is a world point and stays at the world origin. |x0 - x1| = sqrt(3.25); joint m turns about the world z through
    (1, 0 | 0.5 | 1 | 1.5, 0): dx1/dq_m = z x (0, 1.5 - o_m, 0) = (-(1.5 - o_m), 0, 0), g_m = -u_x * that."""
    Rz = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    ref = CollisionReference(PLANAR, [(None, (0, 0, 0), 0.1), ("link4", (0, 0, 0), 0.1)], n_planes=1, base=((1, 0, 0), Rz))
    assert ref.links == [-1, 3] and ref.env_mask == 2 and ref.pair_mask[0] == 2
    r = ref.one(np.zeros(4), _env(planes=[((0, 0, -1), (0, 0, 1))]))
    L = np.sqrt(3.25)
    assert np.abs(r["centres"] - [[0, 0, 0], [1, 1.5, 0]]).max() < 1e-15
    s = r["self"]
    assert abs(s["distance"] - (L - 0.2)) < 1e-15 and s["index"] == 1
    u = np.array([-1, -1.5, 0]) / L
    assert np.abs(s["normal"] - u).max() < 1e-15
    assert np.abs(s["gradient"] - [-u[0] * -(1.5 - o) for o in (0, 0.5, 1.0, 1.5)]).max() < 1e-15
    # the world sphere is not tested against the plane by default: the only candidate is the arm's
    assert r["plane"]["index"] == 1 and abs(r["plane"]["distance"] - 0.9) < 1e-15


# ---------------------------------------------------------------------------------------------- rules
def test_the_first_strict_minimum_wins():
    spheres = [("link4", (0.25, 0, 0), 0.1), ("link4", (0.25, 0, 0), 0.1), ("link2", (0, 0, 0), 0.1), ("link2", (0, 0, 0), 0.1)]
    plane = ((0, -0.5, 0), (0, 1, 0))
    ref = CollisionReference(PLANAR, spheres, n_planes=2, n_obstacles=2, pair_mask=[0b1100, 0b1100, 0, 0] + [0] * 12)
    r = ref.one(np.array([0.3, -0.2, 0.5, 0.1]), _env(planes=[plane, plane], obstacles=[((0, 3, 0), 0.2), ((0, 3, 0), 0.2)]))
    # two identical planes, two identical obstacles, identical spheres: plane 0 / obstacle 0 and the first sphere, the first pair
    assert r["plane"]["index"] == 2 and r["obstacle"]["index"] == 0 and r["self"]["index"] == 16 * 0 + 2
    assert r["plane"]["gap"] == 0.0 and r["obstacle"]["gap"] == 0.0 and r["self"]["gap"] == 0.0


def test_the_empty_category():
    ref = CollisionReference(PLANAR, [("link4", (0, 0, 0), 0.1)], margins=(1e9, 1e9, 1e9))
    r = ref.one(np.zeros(4), _env())
    for cat in ("plane", "obstacle", "self"):
        c = r[cat]
        assert c["distance"] == np.inf and c["index"] == -1 and not c["normal"].any() and not c["gradient"].any()
    assert r["flags"] == 0
    # a mask that tests nothing empties a category that has planes
    ref = CollisionReference(PLANAR, [("link4", (0, 0, 0), 0.1)], n_planes=1, env_mask=0)
    assert ref.one(np.zeros(4), _env(planes=[((0, 0, 0), (0, 0, 1))]))["plane"]["index"] == -1


@pytest.mark.parametrize("where", range(6))
def test_a_nan_plane_is_absent(where):
    ref = CollisionReference(PLANAR, [("link4", (0, 0, 0), 0.1), ("link2", (0, 0, 0), 0.1)], n_planes=2, n_obstacles=1, margins=(10, 10, 0))
    near, far = ((0, -0.5, 0), (0, 1, 0)), ((0, -2.0, 0), (0, 1, 0))
    env = _env(planes=[near, far], obstacles=[((0, 3, 0), 0.2)])
    q = np.array([0.3, -0.2, 0.5, 0.1])
    assert ref.one(q, env)["plane"]["index"] >> 4 == 0
    env[where] = np.nan
    r = ref.one(q, env)
    assert r["plane"]["index"] >> 4 == 1 and np.isfinite(r["plane"]["distance"]) and np.array_equal(r["plane"]["normal"], [0, 1, 0])
    env[6 + where] = np.nan
    r = ref.one(q, env)
    assert r["plane"]["index"] == -1 and r["plane"]["distance"] == np.inf and r["flags"] == 2
    env[12 + where % 4] = np.nan
    assert ref.one(q, env)["flags"] == 0
    # a q that is not finite: that bit alone
    q[2] = np.nan
    assert ref.one(q, _env(planes=[near, far], obstacles=[((0, 3, 0), 0.2)]))["flags"] == 8


def test_the_default_masks():
    env, pairs = default_masks([-1, 0, 1, 2, 2, 5])
    assert env == 0b111110
    assert pairs[:6] == [0b111100, 0b111000, 0b100000, 0b100000, 0b100000, 0] and not any(pairs[6:])


# ---------------------------------------------------------------------------------------------- the gradient
def _hp_distance(model, ref, env, cat, idx, q):
    pos, _ = model.poses(q)

    def centre(k):
        name, c, _ = ref.spheres[k]
        if name is None:
            return hp.M_(c)
        R, p, _ = pos[name]
        return p + R @ hp.M_(c)

    a, k = idx >> 4, idx & 15
    r = [mpf(s[2]) for s in ref.spheres]
    if cat == "plane":
        p0, n = hp.M_(env[6 * a : 6 * a + 3]), hp.M_(env[6 * a + 3 : 6 * a + 6])
        return n @ (centre(k) - p0) - r[k]
    if cat == "obstacle":
        w = hp.M_(env[6 * ref.P + 4 * a : 6 * ref.P + 4 * a + 4])
        e = centre(k) - w[:3]
        return mp.sqrt(e @ e) - r[k] - w[3]
    e = centre(a) - centre(k)
    return mp.sqrt(e @ e) - r[a] - r[k]


@pytest.mark.parametrize("cell", [cc.CELLS[3], cc.CELLS[7], cc.CELLS[12], cc.CELLS[17], cc.CELLS[2]], ids=lambda c: f"{c[0]}-{c[2]}")
def test_the_gradient_is_the_derivative_of_the_distance(cell):
    """planar_4r, six_r (folded axes), Panda, sliding_base (a prismatic joint) and a pitched base; three robots of each"""
    case, ev = cc.evaluated(cell)
    ref, n = case["reference"], case["n"]
    model = hp.Model(cc.model(cell[0])[2], base=case["base"])
    h = mpf(10) ** -10
    worst, checked = 0.0, 0
    for b in (0, 1, cell[1] - 1):
        env = case["env"][:, b] if case["env"] is not None else np.zeros(0)
        q = hp.M_(case["q"][:, b])
        one = ref.one(case["q"][:, b], env)
        for cat in ("plane", "obstacle", "self"):
            idx = one[cat]["index"]
            if idx < 0:
                continue
            # the float64 distance is the 40-digit one
            assert abs(float(_hp_distance(model, ref, env, cat, idx, q)) - one[cat]["distance"]) < 1e-12
            for m in range(n):
                qp, qm = q.copy(), q.copy()
                qp[m], qm[m] = q[m] + h, q[m] - h
                d = (_hp_distance(model, ref, env, cat, idx, qp) - _hp_distance(model, ref, env, cat, idx, qm)) / (2 * h)
                worst = max(worst, abs(float(d) - one[cat]["gradient"][m]))
            checked += 1
    print(f"{cell[0]}: {checked} minima, worst |g - dD/dq| = {worst:.2e}")
    assert checked >= 3 and worst < 1e-12


# ---------------------------------------------------------------------------------------------- the GPU tests' inputs
@pytest.mark.parametrize("cell", cc.DRAWN_CELLS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-P{c[3]}-O{c[4]}-{c[5]}")
def test_every_drawn_cell_is_well_separated(cell):
    """every robot of every cell, none left out: the runner-up of each category is more than 1e-9 m above the winner, each
    |d_min - margin| is above 1e-9, every centre distance that is normalised is above 1e-3 m. If a seed violates it, the seed
    changes, not the assertion."""
    _, ev = cc.evaluated(cell)
    assert ev["gap"].shape == (3, cell[1]) and (ev["gap"] > 1e-9).all(), np.argwhere(~(ev["gap"] > 1e-9))
    assert (np.abs(ev["distance"] - np.array(cc.MARGINS)[:, None]) > 1e-9).all()
    assert (ev["norm"] > 1e-3).all()


def test_the_cells_cover_what_the_gpu_tests_promise():
    C = cc.CELLS
    assert {c[0] for c in C} == set(cc.ROBOTS) and {c[1] for c in C} == {1, 63, 64, 65, 200, 4099}
    assert {c[2] for c in C} == {"last", "arm", "full16"} and {c[3] for c in C} == {0, 1, 2} and {c[4] for c in C} >= {0, 1, 4}
    assert {c[5] for c in C} == {"none", "default", "all"} and any(c[6] for c in C) and any(c[7] for c in C) and any(c[8] for c in C)
    assert all({c[1] for c in C if c[0] == r} >= set(cc.BATCHES) for r in cc.ROBOTS)
    full = cc.draw(next(c for c in C if c[2] == "full16"))
    assert len(full["idx"]) == 16 and -1 in full["idx"] and full["n"] - 1 in full["idx"] and any(0 <= i < full["n"] - 1 for i in full["idx"])

"""Pins tests/body_contact_reference.py, the numpy statement of the whole-arm contact (include/sai2b.h "whole-arm contact") that the
GPU tests and the CPU run of the law's header are held to. No GPU, nothing of the product's law.

1: the batched walk of the URDF chain equals CollisionReference.centres / point_jacobian, robot by robot.
2: known answers: a sphere at rest in a plane gives k delta n and J_c^T of it; one obstacle; a frictionless self pair gives zero
   torque on every joint at or below the lower of its two links; the power identity tb . dq = sum F . v_rel to rounding; mu = d = 0 gives no
   tangential force; NaN and absent entries, k = 0, rows that are not >= 0.
3: every cell the GPU tests draw (tests/body_contact_cases.py): the state stays finite and every penetration stays below the
   smallest sphere radius over the whole run; at least a quarter of the robots have f_n > 0 in some substep, at least a tenth
   never touch, at least one has two candidates active at once; and what the exact comparisons of the GPU tests hang on is well
   separated at every period's end (the deepest candidate 1e-9 ahead of the runner-up, no penetration within 1e-9 of zero, no
   damping factor 1 - d vn within 1e-6 of zero)."""
import math

import numpy as np
import pytest

import body_contact_cases as bc
import collision_cases as cc
from body_contact_reference import ALL, OBSTACLE, PLANE, SELF, BodyContactReference, point_force
from collision_reference import CollisionReference


def _reference(robot, spheres, P=0, O=0, B=1, rows=None, cats=ALL, pair_mask=None, v_eps=1e-3):
    m, _, text = cc.model(robot)
    col = CollisionReference(text, spheres, P, O, pair_mask=pair_mask)
    rows = np.tile([[2e4], [0.0], [0.0]], (1, B)) if rows is None else rows
    return BodyContactReference(col, m, B, rows, categories=cats, v_eps=v_eps, plant=object()), col, m


@pytest.mark.parametrize("robot", cc.ROBOTS)
def test_the_batched_chain_walk_is_the_collision_references(robot):
    spheres = cc.geometry(robot, "full16")
    ref, col, m = _reference(robot, spheres, B=5)
    n = int(m.dof)
    rng = np.random.default_rng(5)
    q = rng.uniform(-1.0, 1.0, (n, 5))
    x, links, axes, origins, types = ref.kinematics(q)
    for b in range(5):
        assert np.abs(x[:, b] - col.centres(q[:, b])).max() < 1e-14
        for k in range(len(spheres)):
            J = ref._jacobian(x[k], links[k], axes, origins, types)[b]
            assert np.abs(J - col.point_jacobian(q[:, b], k)).max() < 1e-14, (robot, b, k)


def _panda_one_sphere():
    names = cc.moving_links("panda")
    spheres = [(names[-1], np.array([0.01, -0.02, 0.03]), 0.05)]
    q = np.array([[0.3], [-0.4], [0.2], [-1.9], [0.1], [1.7], [0.5]])
    return names, spheres, q


def test_a_sphere_at_rest_in_a_plane_is_pushed_by_k_delta_n():
    names, spheres, q = _panda_one_sphere()
    ref, col, m = _reference("panda", spheres, P=1)
    x = col.centres(q[:, 0])[0]
    nrm = np.array([0.0, 0.6, 0.8])
    delta = 5e-3
    env = np.concatenate([x - nrm * (0.05 - delta), nrm])[:, None]
    f = ref.forces(q, np.zeros((7, 1)), env)
    (cat, idx, d, fn, F), = f["candidates"]
    assert (cat, idx) == ("plane", 0) and abs(d[0] - delta) < 1e-15 and abs(fn[0] - 2e4 * delta) < 1e-10
    assert np.abs(F[0] - 2e4 * delta * nrm).max() < 1e-10
    # tb = J_c^T F with the chain's own Jacobian of the application point c = x - r n, given in the link's frame
    R = col.chain.poses(q[:, 0])[0][names[-1]][0]
    J, xc, _ = col.chain.jacobian(q[:, 0], names[-1], spheres[0][1] + R.T @ (-0.05 * nrm))
    assert np.abs(xc - (x - 0.05 * nrm)).max() < 1e-15
    assert np.abs(f["tau"][:, 0] - J[:3].T @ (2e4 * delta * nrm)).max() < 1e-12
    assert f["depth"][0, 0] == d[0] and f["index"][0, 0] == 0 and f["index"][1, 0] == -1 and f["normal_force"][0, 0] == fn[0]


def test_one_obstacle_pushes_along_the_line_of_centres():
    _, spheres, q = _panda_one_sphere()
    ref, col, _ = _reference("panda", spheres, O=1)
    x = col.centres(q[:, 0])[0]
    delta, ro = 8e-3, 0.1
    env = np.concatenate([x + np.array([0.05 + ro - delta, 0, 0]), [ro]])[:, None]
    f = ref.forces(q, np.zeros((7, 1)), env)
    (cat, idx, d, fn, F), = f["candidates"]
    assert cat == "obstacle" and abs(d[0] - delta) < 1e-15 and np.abs(F[0] - 2e4 * delta * np.array([-1.0, 0, 0])).max() < 1e-9
    # the centres coincide: a zero norm gives no force
    env[:3, 0] = x
    f = ref.forces(q, np.zeros((7, 1)), env)
    assert f["candidates"][0][3][0] == 0 and not f["tau"].any() and f["index"][1, 0] == -1


def test_a_self_pair_leaves_the_joints_below_both_links_alone():
    for robot in ("six_r", "sliding_base", "panda"):
        pool = bc._pool(robot)
        q = np.ascontiguousarray(np.concatenate([pool["touch"], pool["double"]], axis=1)[:, :8])
        B = q.shape[1]
        m, _, text = cc.model(robot)
        n = int(m.dof)
        col = CollisionReference(text, cc.geometry(robot, "arm"), pair_mask=bc.pair_mask(robot))
        # without friction: F and -F along u at two points that differ by delta u are in balance. (With friction the two
        # application points, delta apart, leave the couple delta u x F_t: the law applies F where each sphere is touched.)
        rows = np.tile([[2e4], [0.2], [0.0]], (1, B))
        ref = BodyContactReference(col, m, B, rows, categories=SELF, plant=object())
        dq = np.random.default_rng(1).uniform(-1, 1, (n, B))
        f = ref.forces(q, dq)
        assert (f["normal_force"][2] > 0).all()
        for b in range(B):
            low = min(min(col.links[idx >> 4], col.links[idx & 15]) for _, idx, _, fn, _ in f["candidates"] if fn[b] > 0)
            scale = np.abs(f["tau"][:, b]).max()
            assert scale > 1e-3 and np.abs(f["tau"][: low + 1, b]).max() < 1e-12 * max(1.0, f["normal_force"][2, b]), (robot, b)


def test_mu_and_d_zero_give_no_tangential_force_and_power_balances():
    seen = 0
    for cell in bc.CELLS[:20]:
        case, run = bc.ran(cell)
        for f, qd in zip(run["reports"], run["dq"]):
            # the power identity: tb . dq = sum F . v_rel, to rounding
            p = np.sum(f["tau"] * qd, axis=0)
            scale = 1.0 + sum(np.abs(np.linalg.norm(F, axis=1)) for *_, F in f["candidates"]) * np.abs(qd).max(axis=0)
            assert (np.abs(p - f["power"]) < 1e-12 * scale).all(), cell
        if not cell[3]:
            for fs in run["substeps"]:
                for cat, idx, delta, fn, F in fs["candidates"]:
                    # F = f_n u exactly: its norm is f_n
                    assert np.abs(np.linalg.norm(F, axis=1) - fn).max() <= 1e-12 * max(1.0, fn.max())
                    seen += int((fn > 0).sum())
    assert seen > 100


def test_nan_and_absent_entries_give_no_force():
    _, spheres, q = _panda_one_sphere()
    ref, col, _ = _reference("panda", spheres, P=1, O=1)
    x = col.centres(q[:, 0])[0]
    nrm = np.array([0.0, 0.0, 1.0])
    good = np.concatenate([x - nrm * 0.04, nrm, x + [0.1, 0, 0], [0.06]])
    dq = np.full((7, 1), 0.3)
    f = ref.forces(q, dq, good[:, None])
    assert (f["normal_force"][:2, 0] > 0).all() and np.isfinite(f["tau"]).all()
    for row in range(10):
        env = good.copy()
        env[row] = np.nan
        f = ref.forces(q, dq, env[:, None])
        gone = 0 if row < 6 else 1
        assert f["normal_force"][gone, 0] == 0 and f["index"][gone, 0] == -1 and f["normal_force"][1 - gone, 0] > 0 and np.isfinite(f["tau"]).all()
    for bad in ([np.nan, 0.1, 0.1], [2e4, np.nan, 0.1], [2e4, 0.1, np.nan], [0.0, 0.1, 0.1], [-1.0, 0.1, 0.1], [2e4, -0.1, 0.1]):
        ref.rows = np.array(bad)[:, None]
        f = ref.forces(q, dq, good[:, None])
        assert not f["tau"].any() and not f["normal_force"].any() and (f["depth"][:2, 0] > 0).all()  # the penetration is geometry


def test_point_force_is_the_contact_laws():
    import contact_reference as cr

    rng = np.random.default_rng(3)
    B = 50
    n = rng.normal(size=(B, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    v, delta = rng.normal(size=(B, 3)), rng.uniform(-0.01, 0.02, B)
    k, d, mu = rng.uniform(1e3, 3e4, B), rng.uniform(0, 2.0, B), rng.uniform(0, 1, B)
    fn, F = point_force(n, delta, v, k, d, mu, 1e-3)
    # the plane contact's law with x = -delta n, p0 = 0
    rows = np.concatenate([np.zeros((3, B)), n.T, [k], [d], [mu]])
    d2, fn2, F2 = cr.force_law((-delta[:, None] * n).T, v.T, rows, 1e-3)
    assert np.abs(d2 - delta).max() < 1e-15 and np.abs(fn - fn2).max() < 1e-10 and np.abs(F - F2.T).max() < 1e-10


@pytest.mark.parametrize("cell", bc.DRAWN_CELLS, ids=bc.cell_id)
def test_every_drawn_cell_is_bounded_non_vacuous_and_well_separated(cell):
    case, run = bc.ran(cell)
    B = cell[1]
    rmin = min(s[2] for s in case["spheres"])
    touched, multi, deepest = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool), 0.0
    for f in run["substeps"] + run["reports"]:
        touched |= f["normal_force"].sum(axis=0) > 0
        multi |= f["active"] >= 2
        deepest = max(deepest, f["depth"].max())
    assert all(np.isfinite(q).all() and np.isfinite(dq).all() for q, dq in zip(run["q"], run["dq"])), cell
    assert deepest < rmin, (cell, deepest, rmin)
    assert touched.sum() >= math.ceil(B / 4) and (~touched).sum() >= B // 10 and multi.any(), (cell, touched.sum(), multi.sum())
    k, d, mu = case["rows"]
    for f in run["reports"]:
        per = {c: [] for c in range(3)}
        for cat, idx, delta, fn, F in f["candidates"]:
            per[("plane", "obstacle", "self").index(cat)].append(np.where(delta > 0, delta, 0.0))
            with np.errstate(invalid="ignore"):
                assert not ((np.abs(delta) <= 1e-9) & (delta != 0)).any(), cell  # an exact 0 is a zero norm: no candidate
                assert (fn[delta > 0] >= 1e-6 * (k * delta)[delta > 0]).all(), cell  # 1 - d vn stays away from 0
        for c, ds in per.items():
            if len(ds) >= 2:
                s = np.sort(np.array(ds), axis=0)
                assert ((s[-1] - s[-2] > 1e-9) | (s[-1] == 0)).all(), (cell, c)
    print(f"{bc.cell_id(cell)}: {int(touched.sum())} of {B} touch, {int((~touched).sum())} never, {int(multi.sum())} with two candidates, deepest {deepest * 1e3:.1f} mm")

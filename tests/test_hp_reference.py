"""The 40-digit reference of one control tick (tests/hp_reference.py) and its fixture tests/golden/hp_singular.npz (CPU):
the reference is exact enough (40 and 60 digits agree; regenerating robots reproduces the fixture), it is right where
the project already knows the answer (regular robots: the numpy golden fixtures and urdf_np's M and J), the CPU oracle
meets it within C_ORACLE eps kappa_emp with the same bookkeeping on every robot, and that bound has teeth: errors
planted in the reference are rejected by the same check."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import cases  # noqa: E402
import hp_fixture as hf  # noqa: E402
import hp_reference as hp  # noqa: E402
import make_hp_golden as mg  # noqa: E402
import oracle_lib as ol  # noqa: E402

# The oracle's error to the truth in units of eps * kappa_emp stays below this on every robot of the fixture. Measured:
# at most 2.5 in every cell but six_r_mft6, 64 there on a robot with two singular directions (ratios 1.4e-2 and 4e-4,
# absolute error 2.4e-11). kappa_emp prices one ulp of noise normwise in M, J N_prec, x / R, dq in 16 random directions;
# the worst rank-one direction u_5 v_5^T of J N_prec moves that robot's torque 3x more than the random ones do. The GPU
# routes are held to the same C
C_ORACLE = 128
# the smallest relative perturbation of alpha the check still rejects on some robot of the fixture (planted, measured)
ALPHA_DETECTED = 1e-11


@pytest.fixture(scope="module")
def z():
    return np.load(hf.FIXTURE)


def _truth(cell, d, b, dps=40, hooks=None, ticks=None):
    """the exact ticks of robot b of the fixture (mpf torques)"""
    tasks = mg.truth_tasks(cell)
    model = mg.model_of(hf.CELLS[cell]["robot"])
    kinds = hf.kinds(cell)
    goals = [{k.split("_", 1)[1]: v[:, b] for k, v in d.items() if k.startswith(f"{kind}{t}_")} for t, kind in enumerate(kinds)]
    old = hp.mp.dps
    hp.mp.dps = dps
    hp.HOOKS.clear()
    hp.HOOKS.update(hooks or {})
    try:
        state = hp.new_state(model, tasks)
        return [hp.tick(model, tasks, state, d["q"][k][:, b], d["dq"][:, b], goals)[0] for k in range(ticks or d["q"].shape[0])]
    finally:
        hp.mp.dps = old
        hp.HOOKS.clear()


def _pick(d, mask, k=0, n=4):
    return list(np.flatnonzero(mask[k])[:n])


def test_the_fixture_covers_the_singular_branch(z):
    cov = mg.coverage({k: z[k] for k in z.files})
    assert all(v > 0 for v in cov.values()), cov  # 0 < alpha < 1, alpha = 0, type 1, type 2, a clamped tau_s, two directions
    assert os.path.getsize(hf.FIXTURE) < 551_000  # (no larger than the largest fixture before it, c4_three_level.npz)
    for cell in hf.CELLS:
        d = hf.load(cell, z)
        B = d["dq"].shape[1]
        assert 150 <= B <= 250 and B % 64, (cell, B)
        assert (d["nsing"] > 0).sum() >= 10, cell  # (C4's position task meets the region only at the elbow: 13 robots)


def test_40_and_60_digits_agree_and_regeneration_reproduces_the_fixture(z):
    for cell in hf.CELLS:
        d = hf.load(cell, z)
        for b in (0, int(np.flatnonzero(d["nsing"][0] > 0)[0])):
            t40, t60 = _truth(cell, d, b, 40), _truth(cell, d, b, 60)
            for k, (a, c) in enumerate(zip(t40, t60)):
                scale = max(hp.norm_inf(c), 1)
                assert hp.norm_inf(a - c) / scale < 1e-30, (cell, b, k)
                assert np.array_equal(np.array([float(x) for x in a]), d["tau"][k][:, b]), (cell, b, k)
    # the whole row of one robot, kappa_emp included, from the generator itself
    cell = "sliding_base"
    d = hf.load(cell, z)
    tasks = mg.truth_tasks(cell)
    b = int(np.flatnonzero(d["nsing"][0] > 1)[0])
    goals = [{k.split("_", 1)[1]: v[:, b] for k, v in d.items() if k.startswith(f"{kind}{t}_")} for t, kind in enumerate(hf.kinds(cell))]
    (row,) = mg.evaluate((cell, tasks, d["q"][:, :, b], d["dq"][:, b], goals, b, 40))
    for key in ("tau", "alpha", "nsing", "c1", "c2", "types", "clamped", "branch"):
        assert np.array_equal(np.asarray(row[key], dtype=float), d[key][0][..., b]), key
    assert np.array_equal(np.float32(row["ratio"]), d["ratio"][0][:, b]) and np.float32(row["kappa"]) == d["kappa"][0][b]


def test_the_reference_meets_the_numpy_golden_fixtures_on_regular_robots():
    """make_golden.py's numpy restatement (LAPACK, recursive Newton-Euler) on regular Panda robots of C3 and C4, and the
    numpy URDF reading of tests/urdf_np.py (M, J) for every robot: agreement to rounding"""
    import sai2_primitives_perso_amd as pkg
    import urdf_np

    for name, cell in (("c3_mft_jt", "panda_c3"), ("c4_three_level", "panda_c4")):
        inp, opts, kw, g = cases.load_case(name)
        tasks = mg.truth_tasks(cell)
        model = mg.model_of("panda")
        regular = np.flatnonzero(g["out_ns0"] == 6 if cell == "panda_c3" else g["out_ns0"] == 3)[:4]
        for b in regular:
            goals = []
            for t, (kind, _) in enumerate(inp["tasks"]):
                goals.append({k: np.asarray(v)[:, b] for k, v in inp[f"{kind}{t}"].items()})
            tau, _, _ = hp.tick(model, tasks, hp.new_state(model, tasks), inp["q"][:, b], inp["dq"][:, b], goals)
            tau = np.array([float(x) for x in tau])
            assert hf.rel_err(tau[:, None], g["out_tau"][:, b: b + 1])[0] < 1e-12, (name, b)
    rng = np.random.default_rng(5)
    for robot in ("panda", "planar_4r", "six_r", "sliding_base"):
        model = mg.model_of(robot)
        ch = urdf_np.Chain(mg.urdf_text(robot), is_file=False)
        for _ in range(2):
            q = rng.uniform(-1, 1, model.dof)
            pos, jinfo, M, _ = model.dynamics(hp.M_(q))
            Mn, _ = ch.mass_matrix_and_gravity(q)
            assert np.abs(np.array(M, dtype=float) - Mn).max() < 1e-13 * np.abs(Mn).max(), robot
            link = [l for l in ch.links if ch.links[l] is not None][-1]
            J, _, _ = model.jacobian(pos, jinfo, link, hp.M_([0.01, 0.02, 0.03]))
            Jn, _, _ = ch.jacobian(q, link, [0.01, 0.02, 0.03])
            assert np.abs(np.array(J, dtype=float) - Jn).max() < 1e-14, robot


def _oracle(cell):
    return hf.make(cell, ol.joint_task, ol.motion_force_task, lambda m, cfgs, B: ol.Oracle(m, cfgs, B, threads=8))


@pytest.mark.parametrize("cell", list(hf.CELLS))
def test_the_oracle_meets_the_exact_answer(cell):
    """every robot and tick: error <= C_ORACLE eps kappa_emp, split / c1 / c2 equal to the truth"""
    o, d = _oracle(cell)
    for k, (tau, state) in enumerate(hf.run(o, cell, d)):
        r = hf.ratio_to_bound(tau, d, k)
        assert r.max() <= C_ORACLE, (cell, k, np.argmax(r), r.max())
        assert hf.bookkeeping_mismatch(state, d, k).size == 0, cell


def _rejected(cell, d, robots, hooks):
    """the planted reference's torques, as a kernel's, fail the check of tests/test_gpu_hp_singular.py on a robot"""
    for b in robots:
        for k, tau in enumerate(_truth(cell, d, b, hooks=hooks)):
            tau = np.array([float(x) for x in tau])
            if hf.rel_err(tau[:, None], d["tau"][k][:, b: b + 1])[0] > C_ORACLE * np.finfo(float).eps * d["kappa"][k][b]:
                return True
    return False


def test_planted_errors_are_rejected(z):
    blend = lambda d: (d["alpha"] > 0) & (d["alpha"] < 1) & (d["nsing"] > 0)
    c3 = hf.load("panda_c3", z)
    # alpha off by a relative 1e-8, and the smallest perturbation still caught
    assert _rejected("panda_c3", c3, _pick(c3, blend(c3)), {"alpha_rel": 1e-8})
    assert _rejected("panda_c3", c3, _pick(c3, blend(c3)), {"alpha_rel": ALPHA_DETECTED})
    # the sign of v_s flipped in the type-2 torque; kv_type_1 where kv_type_2 belongs: robots on the type-2 branch
    t2 = blend(c3) & (c3["branch"] == 2)
    assert _rejected("panda_c3", c3, _pick(c3, t2), {"flip_vs_type2": True})
    assert _rejected("panda_c3", c3, _pick(c3, t2), {"kv1_for_kv2": True})
    # the effort clamp of tau_s dropped: robots with a clamped component and alpha > 0
    for cell in hf.CELLS:
        d = hf.load(cell, z)
        cl = blend(d) & (d["clamped"] > 0)
        if cl[0].any():
            assert _rejected(cell, d, _pick(d, cl), {"no_clamp": True}), cell
            break
    else:
        raise AssertionError("no clamped robot in the blending band")
    # q_prior never refreshed (kept at the middle of the joint ranges): robots on the type-1 branch
    seq = hf.load("panda_c3_seq", z)
    t1 = blend(seq) & (seq["branch"] == 1)
    assert _rejected("panda_c3_seq", seq, _pick(seq, t1, n=2), {"stale_q_prior": True})


def test_pinv_for_lambda_s_is_the_inverse_on_every_robot_of_the_fixture(z):
    """pinv in place of inv for Lambda_s is NOT an error the check can see, because it is not an error here: J_s M^-1 J_s^T
    is 1 x 1 or 2 x 2 with a condition number far below the pseudo-inverse's cut-off 1 / (n eps), so its pseudo-inverse
    is its inverse. Full dynamic decoupling, where Lambda_s itself reaches the torque (BIE and impedance use their own
    matrices): the planted reference agrees with the fixture to rounding on every robot of the region"""
    d = hf.load("panda_c3_full", z)
    region = np.flatnonzero((d["alpha"][0] > 0) & (d["nsing"][0] > 0))
    assert region.size > 100
    for b in region:
        (tau,) = _truth("panda_c3_full", d, b, hooks={"pinv_ls": True})
        assert np.array_equal(np.array([float(x) for x in tau]), d["tau"][0][:, b]), b

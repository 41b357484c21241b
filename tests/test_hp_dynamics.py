"""The exact rigid-body dynamics of tests/hp_reference.py and its fixture tests/golden/hp_dynamics.npz (CPU): the bias
vector derived two independent ways (velocity-product accelerations of the bodies; the Lagrangian form from
derivatives of M) agrees with itself and across precisions, regenerating robots reproduces the fixture, the CPU oracle
meets it (bias, gravity, the simulation step, the control tick with gravity compensation on robots with prismatic
joints inside the chain) within the bounds of tests/hp_dynamics_fixture.py, and those bounds have teeth: errors
planted in the reference are rejected by the same check."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import hp_dynamics_fixture as hd  # noqa: E402
import hp_reference as hp  # noqa: E402
import make_hp_dynamics_golden as mg  # noqa: E402
import oracle_lib as ol  # noqa: E402

C_BIAS, C_SIM, C_POSE, C_TICK = hd.C_BIAS, hd.C_SIM, hd.C_POSE, hd.C_TICK
EPS = hd.EPS
ALL = list(hd.DYN_CELLS) + list(hd.TICK_CELLS)


@pytest.fixture(scope="module")
def z():
    return np.load(hd.FIXTURE)


def _base(d):
    return (d["base_pos"], d["base_rot"]) if "base_pos" in d else None


def test_the_fixture_is_small_and_complete(z):
    assert os.path.getsize(hd.FIXTURE) < 551_000  # (no larger than tests/golden/hp_singular.npz)
    for cell in ALL:
        d = hd.load(cell, z)
        B = d["dq"].shape[1]
        assert B > 64 and B % 64, (cell, B)
        assert np.isfinite(d["kappa" if cell in hd.TICK_CELLS else "cond"]).all(), cell


def test_two_bias_derivations_agree_and_40_and_60_digits_agree(z):
    for cell in hd.DYN_CELLS:
        d = hd.load(cell, z)
        model = mg.model_of(cell, _base(d))
        q, dq = d["q"][:, 0], d["dq"][:, 0]
        for grav in (False, None):
            b, beta = hp.bias_terms(model, q, dq, grav)
            lag = hp.bias_lagrange(model, q, dq, grav)
            assert hp.norm_inf(b - lag) <= 1e-25 * max(hp.norm_inf(beta), 1), (cell, grav)
            old = hp.mp.dps
            hp.mp.dps = 60
            try:
                b60 = hp.bias(model, q, dq, grav)
            finally:
                hp.mp.dps = old
            assert hp.norm_inf(b - b60) <= 1e-30 * max(hp.norm_inf(beta), 1), (cell, grav)


def test_regeneration_reproduces_the_fixture(z):
    """one robot a cell, every array of its row (the float32 scales included), from the generator itself"""
    for cell in hd.DYN_CELLS:
        d = hd.load(cell, z)
        b = d["q"].shape[1] - 1
        row = mg.evaluate_dyn((cell, _base(d), d["q"][:, b], d["dq"][:, b], d["tau"][:, b], 40))
        for k in ("b0", "g"):
            assert np.array_equal(row[k], d[k][:, b]), (cell, k)
        for k in ("beta0", "betag", "cond"):
            assert np.float32(row[k]) == d[k][b], (cell, k)
        for name, *_ in hd.SIMS:
            for k in ("q", "dq") if name != "sim1" else ("dq",):
                assert np.array_equal(row[name][k], d[f"{name}.{k}"][:, b]), (cell, name, k)
            assert np.float32(row[name]["xscale"]) == d[f"{name}.xscale"][b] and np.float32(row[name]["minv"]) == d[f"{name}.minv"][b]
    for cell in hd.TICK_CELLS:
        d = hd.load(cell, z)
        tasks = mg.tick_tasks(cell)
        b = 3
        kinds = [t["kind"] for t in tasks]
        goals = [{k.split("_", 1)[1]: v[:, b] for k, v in d.items() if k.startswith(f"{kind}{t}_")} for t, kind in enumerate(kinds)]
        row = mg.evaluate_tick((cell, tasks, d["q"][:, b], d["dq"][:, b], goals, b, 40, True))
        for k in ("tau", "x", "R", "v", "w"):
            assert np.array_equal(row[k], d[k][:, b]), (cell, k)
        assert np.float32(row["kappa"]) == d["kappa"][b]
        assert np.array_equal(row["sim1"]["dq"], d["sim1.dq"][:, b])


def _dyn_oracle(cell, d):
    m, _ = hd.product_model(cell, d)
    n = d["q"].shape[0]
    return ol.Oracle(m, [ol.joint_task("j", robot_dof=n)], d["q"].shape[1], threads=8)


@pytest.mark.parametrize("cell", list(hd.DYN_CELLS))
def test_the_oracle_meets_the_exact_dynamics(cell, z):
    d = hd.load(cell, z)
    o = _dyn_oracle(cell, d)
    for check, r in hd.dynamics_ratios(o, d).items():
        assert r.max() <= hd.bound(check), (cell, check, int(np.argmax(r)), r.max())


@pytest.mark.parametrize("cell", list(hd.TICK_CELLS))
def test_the_oracle_meets_the_exact_tick_and_period(cell, z):
    """torques within C_TICK eps kappa_emp, the frame pose, then one simulated period under the oracle's own torques"""
    d = hd.load(cell, z)
    o = hd.tick_controller(cell, d, ol.joint_task, ol.motion_force_task, lambda m, cfgs, B: ol.Oracle(m, cfgs, B, threads=8))
    tau = o.tick()
    r = hd.tick_ratio(tau, d)
    assert r.max() <= C_TICK, (cell, int(np.argmax(r)), r.max())
    st = o.get_mft_status(0)
    for check, r in hd.pose_ratios(st["pos"], st["rot"], d).items():
        assert r.max() <= C_POSE, (cell, check, r.max())
    o.sim_step(tau, hd.DT, 1, with_gravity=True)
    q, dq = o.get_state()
    r = hd.sim_ratio(q, dq, d, "sim1", dtau=tau - d["tau"])
    assert r.max() <= C_SIM, (cell, int(np.argmax(r)), r.max())


# ---- planted errors ----

def _planted_dyn(cell, d, robots, hooks):
    """the planted reference's bias and simulated states of the given robots, as a kernel's: {check: ratios}"""
    model = mg.model_of(cell, _base(d))
    hp.HOOKS.clear()
    hp.HOOKS.update(hooks)
    try:
        out = {}
        sub = d["b0"][:, robots], d["beta0"][robots]
        b = np.array([[float(x) for x in hp.bias(model, d["q"][:, k], d["dq"][:, k], False)] for k in robots]).T
        out["bias0"] = hd.bias_ratio(b, *sub)
        rows = []
        for k in robots:
            q, dq = hp.sim_step(model, d["q"][:, k], d["dq"][:, k], d["tau"][:, k], hd.DT, 3, False)
            rows.append(([float(x) for x in q], [float(x) for x in dq]))
        dsub = {key: (v[..., robots] if v.ndim and v.shape[-1] == d["dq"].shape[1] else v) for key, v in d.items()}
        out["sim3"] = hd.sim_ratio(np.array([r[0] for r in rows]).T, np.array([r[1] for r in rows]).T, dsub, "sim3")
        return out
    finally:
        hp.HOOKS.clear()


def test_planted_errors_are_rejected(z):
    robots = [0, 1, 2]
    # the Coriolis acceleration of a sliding frame halved: caught on every robot with a prismatic joint behind a
    # revolute one, and nothing to catch without a prismatic joint (the planted bias is the exact one, bit for bit)
    for cell in ("rprp_4", "stanford_6", "slider_7", "stanford_6_pitch90"):
        r = _planted_dyn(cell, hd.load(cell, z), robots, {"pris_coriolis_half": True})
        assert r["bias0"].max() > C_BIAS and r["sim3"].max() > C_SIM, (cell, r)
    for cell in ("planar_4r", "six_r"):
        d = hd.load(cell, z)
        model = mg.model_of(cell, None)
        hp.HOOKS["pris_coriolis_half"] = True
        try:
            planted = hp.bias(model, d["q"][:, 0], d["dq"][:, 0], False)
        finally:
            hp.HOOKS.clear()
        assert all(a == b for a, b in zip(planted, hp.bias(model, d["q"][:, 0], d["dq"][:, 0], False))), cell
    # no gyroscopic moment w x I w; q stepped with the old velocity (explicit Euler)
    assert any(_planted_dyn(c, hd.load(c, z), robots, {"no_gyroscopic": True})["bias0"].max() > C_BIAS for c in ("panda", "six_r"))
    assert any(_planted_dyn(c, hd.load(c, z), robots, {"explicit_euler": True})["sim3"].max() > C_SIM for c in ("panda", "rprp_4"))

"""The simulation harness and the control tick of robots with prismatic joints inside the chain against the exact
answers of tests/golden/hp_dynamics.npz (-m gpu), under the bounds the CPU oracle is calibrated to in
tests/test_hp_dynamics.py:
  every dynamics cell   get_bias without and with gravity, the three simulation variants of hp_dynamics_fixture.SIMS
  every tick cell       on the routes of test_gpu_hp_singular that apply to regular robots: torques within
                        C_ROUTE eps kappa_emp, fallback_count, the MotionForceTask's pose and velocity, then one
                        simulated period from the resident torques (sim_step(None)) against the exact next state
SAI2B_HP_DYN_REPORT=<file> writes the worst ratio to its bound per (cell, check) as JSON. Reads the fixture only."""
import json
import os

import numpy as np
import pytest

import hp_dynamics_fixture as hd
import sai2_primitives_perso_amd as pkg
from test_gpu_hp_singular import C_ROUTE, ROUTES

pytestmark = pytest.mark.gpu
TICK_ROUTES = ("default", "no_inlane", "generic16", "generic8", "introspection")
_REPORT = {}


def _report(key, ratios):
    _REPORT[key] = {k: float(np.max(v)) for k, v in ratios.items()}
    path = os.environ.get("SAI2B_HP_DYN_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_REPORT, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("cell", list(hd.DYN_CELLS))
def test_simulation_meets_the_exact_dynamics(cell):
    d = hd.load(cell)
    m, _ = hd.product_model(cell, d)
    n, B = d["q"].shape
    g = pkg.Controller(m, [pkg.joint_task_config("j", None, robot_dof=n)], B)
    ratios = hd.dynamics_ratios(g, d, gravity=False)
    _report(cell, ratios)
    for check, r in ratios.items():
        assert r.max() <= hd.bound(check), (cell, check, int(np.argmax(r)), r.max())


@pytest.mark.parametrize("route", TICK_ROUTES)
@pytest.mark.parametrize("cell", list(hd.TICK_CELLS))
def test_tick_and_period_meet_the_exact_answer(cell, route, monkeypatch):
    d = hd.load(cell)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    try:
        g = hd.tick_controller(cell, d, pkg.joint_task_config, pkg.motion_force_task_config,
                               lambda m, cfgs, B: pkg.Controller(m, cfgs, B, introspection=route == "introspection"))
    finally:
        for k in ROUTES[route]:
            monkeypatch.delenv(k)
    B = d["dq"].shape[1]
    tau = g.tick()
    fb = g.fallback_count()
    ratios = dict(tau=hd.tick_ratio(tau, d))
    # every robot is regular: the default route keeps them all (slack as test_gpu_hp_singular._route_ran), the
    # generic routes run every one through the work list
    if route == "default":
        assert fb <= 2 + B // 100, (cell, route, fb)
    elif route in ("generic16", "generic8"):
        assert fb == B, (cell, route, fb)
    st = g.get_mft_status(0)
    v, w = g.get_mft_velocity(0)
    ratios.update(hd.pose_ratios(st["pos"], st["rot"], d, v, w))
    g.sim_step(None, hd.DT, 1, with_gravity=True)
    q, dq = g.get_state()
    ratios["sim1"] = hd.sim_ratio(q, dq, d, "sim1", dtau=tau - d["tau"])
    _report(f"{cell}/{route}", ratios)
    for check, r in ratios.items():
        assert r.max() <= (C_ROUTE if check == "tau" else hd.bound(check)), (cell, route, check, int(np.argmax(r)), r.max())

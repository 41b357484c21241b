"""Every kernel route on the robots of the exact-answer fixture tests/golden/hp_force.npz (-m gpu): the force and moment
spaces in the world or the compliant frame, the goal and the sensed wrench through the sensor frame, open and closed
loop with integrators and the feedback limit, the feed-forward gains, the motion integrators, velocity saturation and
per-axis gains, and the JointTask's integrator and saturation, in and around the singularity-blending region, where
F_f enters as J_x^T (Lambda_x U_x^T F_u + U_x^T F_f) and decides the type-2 direction through ||F_u + F_f||.

For every robot and every tick: torques within C_ROUTE eps kappa of the 40-digit truth of tests/hp_reference.py, the
integrators (tests/plumbing.integrators) within C_ROUTE eps kappa_integ of the exact ones, the rows of a loop that is
off exactly where they were, singular directions, c1 and c2 equal to the truth's, and the route asked for really ran.
No robot is exempt: the generator keeps every robot 1e-6 away from each decision, the four norm thresholds and the
JointTask's per-joint saturation included.

Routes and cells as tests/test_gpu_hp_singular.py builds them (its ROUTES, switches set before the controller is
created): the Panda C3 cells run default, no_fast, sing6, generic16, generic8 and introspection; the others default,
no_inlane, sing6 where the hierarchy has a 6-row task, generic16, generic8 and introspection; once per cell the split
calls update_task_models + compute_control_torques.

SAI2B_HP_REPORT=<file> writes per (cell, route) the max error / (eps kappa), the same for the integrators and the max
absolute error, as JSON (merged into what the file holds: tests/test_hp_force_reference.py writes its "oracle" key)."""
import numpy as np
import pytest

import hp_fixture as hf
import hp_force_fixture as ff
import sai2_primitives_perso_amd as pkg
from test_gpu_hp_singular import C_ROUTE, ROUTES, _route_ran

pytestmark = pytest.mark.gpu

# the cell of tests/hp_fixture.py with the same robot and hierarchy: what _route_ran knows a cell by
SIBLING = {c: {"c3": "panda_c3", "c4": "panda_c4"}.get(v["hier"], v["hier"]) for c, v in ff.CELLS.items()}
PANDA_C3 = [c for c, v in ff.CELLS.items() if v["hier"] == "c3"]
SIX_ROW = [c for c, v in ff.CELLS.items() if v["hier"] in ("c3", "six_r_mft6", "sliding_base")]


def _cells():
    for cell in ff.CELLS:
        panda3 = cell in PANDA_C3
        for route in ROUTES:
            if route == "no_fast" and not panda3 or route == "no_inlane" and panda3 or route == "sing6" and cell not in SIX_ROW:
                continue
            yield cell, route


def _controller(cell, route, monkeypatch):
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    try:
        return ff.make(cell, pkg.joint_task_config, pkg.motion_force_task_config,
                       lambda m, cfgs, B: pkg.Controller(m, cfgs, B, introspection=route == "introspection"))
    finally:
        for k in ROUTES[route]:
            monkeypatch.delenv(k)


def _check(cell, route, results, d, fbs=None):
    B = d["dq"].shape[1]
    mft = next(o for o, k in zip(ff.CELLS[cell]["opts"], ff.kinds(cell)) if k == "mft")
    worst = worst_i = worst_abs = 0.0
    for k, (tau, state, integ) in enumerate(results):
        r = hf.ratio_to_bound(tau, d, k)
        ri = ff.integ_ratio(integ, d, k)
        print(cell, route, "tick", k, "max ratio", r.max(), "integrators", ri.max(axis=1), "max abs", np.abs(tau - d["tau"][k]).max())
        bad = np.flatnonzero(r > C_ROUTE)
        assert bad.size == 0, (cell, route, k, bad[:8], r[bad][:8], d["kappa"][k][bad][:8], d["nsing"][k][bad][:8])
        bad = np.flatnonzero(ri.max(axis=0) > C_ROUTE)
        assert bad.size == 0, (cell, route, k, bad[:8], ri[:, bad[:8]], integ[0][:, bad[:2]], d["mft_integ"][k][:, bad[:2]])
        for on, rows in ((mft.get("closed_loop_force"), slice(6, 9)), (mft.get("closed_loop_moment"), slice(9, 12))):
            if not on:  # every tick starts from the controller's construction: the rows were zero
                assert not integ[0][rows].any(), (cell, route, k, rows)
        mism = hf.bookkeeping_mismatch(state, d, k)
        assert mism.size == 0, (cell, route, k, mism[:8], [s[mism][:4] for s in state], d["nsing"][k][mism][:4],
                                d["c1"][k][mism][:4], d["c2"][k][mism][:4])
        if fbs is not None:
            _route_ran(SIBLING[cell], route, fbs[k], d, k, B)
        worst, worst_i = max(worst, float(r.max())), max(worst_i, float(ri.max()))
        worst_abs = max(worst_abs, float(np.abs(tau - d["tau"][k]).max()))
    ff.report({f"{cell}/{route}": dict(in_region=int((d["nsing"] > 0).sum()), robot_ticks=int(d["nsing"].size), max_ratio=worst,
                                       max_ratio_integ=worst_i, max_abs=worst_abs)})


@pytest.mark.parametrize("cell,route", list(_cells()))
def test_route_meets_the_exact_answer(cell, route, monkeypatch):
    g, d = _controller(cell, route, monkeypatch)
    fbs = []

    def tick(c):
        tau = c.tick()
        fbs.append(c.fallback_count())
        return tau

    results = ff.run(g, cell, d, tick)
    _check(cell, route, results, d, None if route == "introspection" else fbs)


@pytest.mark.parametrize("cell", list(ff.CELLS))
def test_split_calls_meet_the_exact_answer(cell, monkeypatch):
    """update_task_models() then compute_control_torques(): the same bounds and bookkeeping"""
    g, d = _controller(cell, "default", monkeypatch)

    def tick(c):
        c.update_task_models()
        return c.compute_control_torques()

    _check(cell, "split", ff.run(g, cell, d, tick), d)

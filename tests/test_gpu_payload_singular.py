"""Per-robot payloads inside a singularity-blending region (-m gpu): the robots of tests/golden/hp_payload.npz (32 poses of
tests/singular_poses.py, two payloads alternating) on every kernel route, held to the bound tests/test_gpu_hp_singular.py
applies, C_ROUTE eps kappa_emp with the 40-digit torques and kappa_emp of the fixture, and to the fixture's singularity
bookkeeping; and, where the MotionForceTask is the first task, each robot's route, as the work-list count and the singularity
state show it, is the one it takes without a payload (kinematics, Jacobians and the singularity certificate never read
inertial parameters). Behind a JointTask (the sliding-base Panda) the task's singular values are those of J N_prec, whose
dynamically consistent N_prec is built with M, so there a payload legitimately moves robots across the edge of the region:
that cell is held to the exact answer and its bookkeeping only."""
import numpy as np
import pytest

import hp_fixture as hf
import payload_cases as pc
import sai2_primitives_perso_amd as pkg
from test_gpu_hp_singular import C_ROUTE, ROUTES

pytestmark = pytest.mark.gpu

CASES = [(cell, route) for cell in pc.HP_CELLS for route in ("default", "no_inlane", "sing6", "generic16", "generic8", "introspection")
         if not (route == "sing6" and cell == "six_r")]


def _controller(cell, route, d, monkeypatch, payload):
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    try:
        g = pc.hp_make(cell, d, pkg.joint_task_config, pkg.motion_force_task_config,
                       lambda m, cfgs, B: pkg.Controller(m, cfgs, B, introspection=route == "introspection"))
    finally:
        for k in ROUTES[route]:
            monkeypatch.delenv(k)
    if payload:
        link, rows = pc.hp_rows(cell, d["dq"].shape[1])
        g.set_link_payload(link, *rows)
    return g


@pytest.mark.parametrize("cell,route", CASES)
def test_route_with_payloads_meets_the_exact_answer_and_takes_the_same_route(cell, route, monkeypatch):
    d = pc.hp_load(cell)
    B = d["dq"].shape[1]
    t = hf.kinds(cell).index("mft")
    out = {}
    for payload in (True, False):
        g = _controller(cell, route, d, monkeypatch, payload)
        g.set_state(np.ascontiguousarray(d["q"][0]), np.ascontiguousarray(d["dq"]))
        tau = g.tick()
        out[payload] = (tau, g.fallback_count(), [np.asarray(s).astype(int) for s in g.get_mft_singularity_state(t)])
    tau, fb, state = out[True]
    r = hf.ratio_to_bound(tau, d, 0)
    print(f"{cell}/{route}: in region {int((d['nsing'][0] > 0).sum())} of {B}, max error {r.max():.3f} eps kappa, work list {fb}")
    assert (d["nsing"][0] > 0).sum() >= B // 4  # the singular branches run
    assert r.max() <= C_ROUTE, (cell, route, np.flatnonzero(r > C_ROUTE), r.max())
    assert hf.bookkeeping_mismatch(tuple(state), d, 0).size == 0
    # the same route without the payload, robot by robot; and the payload is not a no-op here either
    if cell in pc.HP_FIRST_TASK:
        assert fb == out[False][1], (fb, out[False][1])
        for a, b in zip(state, out[False][2]):
            assert np.array_equal(a, b)
    assert hf.rel_err(out[False][0], d["tau"][0]).max() > 1e-6
    if route in ("generic16", "generic8"):
        assert fb == B
    elif route == "no_inlane":
        assert fb >= (d["nsing"][0] > 0).sum()
    elif (route == "default" and cell == "six_r") or route == "sing6":
        assert fb <= (d["nsing"][0] > 1).sum() + 2  # one singular direction stays in the lane

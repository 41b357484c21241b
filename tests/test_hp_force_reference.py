"""The 40-digit reference of the force, integral and saturation laws (tests/hp_reference.py) and its fixture
tests/golden/hp_force.npz (CPU), as tests/test_hp_reference.py does for the plain motion law: the fixture covers what it
must, 40 and 60 digits agree and regeneration reproduces the committed numbers, the reference meets the numpy golden
fixtures of these laws on their regular robots, the CPU oracle meets the exact torques and integrators within
C_ORACLE eps kappa on every robot and tick with the same bookkeeping, and every error planted in the reference's new
laws is rejected by that check."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import cases  # noqa: E402
import hp_fixture as hf  # noqa: E402
import hp_force_fixture as ff  # noqa: E402
import hp_reference as hp  # noqa: E402
import make_hp_force_golden as mfg  # noqa: E402
import make_hp_golden as mg  # noqa: E402
import oracle_lib as ol  # noqa: E402
from test_hp_reference import C_ORACLE  # noqa: E402  (the project's 128: imported, not redefined)

EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def z():
    return np.load(ff.FIXTURE)


def _goals(cell, d, b):
    return [{k.split("_", 1)[1]: v[:, b] for k, v in d.items() if k.startswith(f"{kind}{t}_")} for t, kind in enumerate(ff.kinds(cell))]


_TASKS = {}


def _truth(cell, d, b, dps=40, hooks=None):
    """the exact ticks of robot b of the fixture: per tick (mpf torques, integrator groups)"""
    if cell not in _TASKS:
        _TASKS[cell] = mfg.truth_tasks(cell)
    tasks = _TASKS[cell]
    model = mg.model_of(ff.CELLS[cell]["robot"])
    old = hp.mp.dps
    hp.mp.dps = dps
    hp.HOOKS.clear()
    hp.HOOKS.update(hooks or {})
    try:
        state = hp.new_state(model, tasks)
        out = []
        for k in range(d["q"].shape[0]):
            tau, info, _ = hp.tick(model, tasks, state, d["q"][k][:, b], d["dq"][:, b], _goals(cell, d, b))
            out.append((tau, hp.integ_groups(tasks, info)))
        return out
    finally:
        hp.mp.dps = old
        hp.HOOKS.clear()


def test_the_fixture_covers_the_laws_and_the_singular_branch(z):
    cov = mfg.coverage({k: z[k] for k in z.files})
    assert all(v > 0 for v in cov.values()), cov
    assert os.path.getsize(ff.FIXTURE) < 551_000
    assert sorted({k.split(".")[0] for k in z.files}) == sorted(ff.CELLS)
    for cell, c in ff.CELLS.items():
        d = ff.load(cell, z)
        B = d["dq"].shape[1]
        assert B == c["B"] and 67 <= B <= 131 and B % 64 and B > 64, (cell, B)
        assert d["tau"].shape[0] == c["ticks"] and (d["nsing"] > 0).sum() >= 5, cell


def test_40_and_60_digits_agree_and_regeneration_reproduces_the_fixture(z):
    for cell in ff.CELLS:
        d = ff.load(cell, z)
        for b in (0, int(np.flatnonzero(d["nsing"][0] > 0)[0])):
            for k, ((a, ia), (c, ic)) in enumerate(zip(_truth(cell, d, b, 40), _truth(cell, d, b, 60))):
                assert hp.norm_inf(a - c) / max(hp.norm_inf(c), 1) < 1e-30, (cell, b, k)
                ia, ic = np.concatenate(ia), np.concatenate(ic)
                assert hp.norm_inf(ia - ic) < 1e-30, (cell, b, k)
                assert np.array_equal(np.array([float(x) for x in a]), d["tau"][k][:, b]), (cell, b, k)
                assert np.array_equal(np.array([float(x) for x in ia]), np.concatenate([d["mft_integ"][k][:, b], d["jt_integ"][k][:, b]]))
    # the whole rows of one robot, both condition numbers included, from the generator itself
    cell = "panda_c3_closed"
    d = ff.load(cell, z)
    b = int(np.flatnonzero(d["nsing"][0] > 0)[1])
    rows = mfg.evaluate((cell, mfg.truth_tasks(cell), d["q"][:, :, b], d["dq"][:, b], _goals(cell, d, b), b, 40))
    for k, row in enumerate(rows):
        for key in ("tau", "alpha", "nsing", "c1", "c2", "types", "clamped", "branch", "mft_integ", "jt_integ") + ff.SATS:
            assert np.array_equal(np.asarray(row[key], dtype=float), d[key][k][..., b]), (key, k)
        for key in ("ratio", "kappa", "kappa_integ", "ff"):
            assert np.array_equal(np.float32(row[key]), d[key][k][..., b]), (key, k)


@pytest.mark.parametrize("name", ["c3_force_open_loop", "c3_force_closed_loop", "c3_integral_3ticks", "c3_velocity_saturation"])
def test_the_reference_meets_the_numpy_golden_fixtures_on_regular_robots(name):
    """make_golden.py's numpy restatement of the same laws (written apart from this one) on regular Panda robots, every
    tick of the case: the last tick's torques to 1e-12"""
    import sai2_primitives_perso_amd as pkg

    inp, opts, kw, g = cases.load_case(name)
    cfgs = [cases.apply_opts(c, o) for c, o in zip(pkg.task_configs(inp["tasks"]), opts)]
    tasks = mfg.config_tasks(cfgs, hf.hierarchy("c3", 7))
    model = mg.model_of("panda")
    regular = np.flatnonzero(g["out_ns0"] == 6)[:4]
    assert regular.size == 4
    for b in regular:
        goals = [{k: np.asarray(v)[:, b] for k, v in inp[f"{kind}{t}"].items()} for t, (kind, _) in enumerate(inp["tasks"])]
        if "in_wrench_f" in g:
            goals[0].update({k: g[f"in_wrench_{k}"][:, b] for k in ff.WRENCH})
        state = hp.new_state(model, tasks)
        for _ in range(kw.get("ticks", 1)):
            tau, _, _ = hp.tick(model, tasks, state, inp["q"][:, b], inp["dq"][:, b], goals)
        tau = np.array([float(x) for x in tau])
        assert hf.rel_err(tau[:, None], g["out_tau"][:, b: b + 1])[0] < 1e-12, (name, b)


@pytest.mark.parametrize("cell", list(ff.CELLS))
def test_the_oracle_meets_the_exact_answer(cell):
    """every robot and tick: torques within C_ORACLE eps kappa, integrators within C_ORACLE eps kappa_integ, the rows of a
    loop that is off untouched, split / c1 / c2 equal to the truth. SAI2B_HP_REPORT=<file> writes the max ratios"""
    o, d = ff.make(cell, ol.joint_task, ol.motion_force_task, lambda m, cfgs, B: ol.Oracle(m, cfgs, B, threads=8))
    mft = next(opt for opt, kind in zip(ff.CELLS[cell]["opts"], ff.kinds(cell)) if kind == "mft")
    worst = worst_i = 0.0
    for k, (tau, state, integ) in enumerate(ff.run(o, cell, d)):
        r = hf.ratio_to_bound(tau, d, k)
        ri = ff.integ_ratio(integ, d, k)
        print(cell, k, "max ratio", r.max(), "integrators", ri.max(axis=1))
        assert r.max() <= C_ORACLE, (cell, k, np.argmax(r), r.max())
        assert ri.max() <= C_ORACLE, (cell, k, ri.max(axis=1))
        for on, rows in ((mft.get("closed_loop_force"), slice(6, 9)), (mft.get("closed_loop_moment"), slice(9, 12))):
            if not on:  # the controller is new and its integrators zero: a loop that is off leaves its rows there
                assert not integ[0][rows].any(), (cell, k, rows)
        assert hf.bookkeeping_mismatch(state, d, k).size == 0, cell
        worst, worst_i = max(worst, float(r.max())), max(worst_i, float(ri.max()))
    ff.report({cell: dict(max_ratio=worst, max_ratio_integ=worst_i)}, key="oracle")


def _rejected(cell, d, robots, hooks):
    """the planted reference's torques or integrators, as a kernel's, fail the check on one of the robots"""
    assert len(robots), (cell, hooks)
    for b in robots:
        for k, (tau, groups) in enumerate(_truth(cell, d, b, hooks=hooks)):
            tau = np.array([float(x) for x in tau])[:, None]
            if hf.ratio_to_bound(tau, {"tau": d["tau"][:, :, b: b + 1], "kappa": d["kappa"][:, b: b + 1]}, k)[0] > C_ORACLE:
                return True
            mft = np.array([float(x) for g in groups[:4] for x in g])[:, None]
            jt = np.array([float(x) for x in groups[4]])[:, None]
            one = {key: d[key][..., b: b + 1] for key in ("mft_integ", "jt_integ", "kappa_integ")}
            if ff.integ_ratio((mft, jt), one, k).max() > C_ORACLE:
                return True
    return False


def _pick(mask, n=3):
    """robots for which the mask holds at some tick"""
    return list(np.flatnonzero(mask.any(axis=0))[:n])


def test_planted_errors_are_rejected(z):
    d = {cell: ff.load(cell, z) for cell in ff.CELLS}
    every = lambda c: np.ones_like(d[c]["alpha"], dtype=bool)
    t2 = lambda c: (d[c]["branch"] == 2) & (d[c]["alpha"] < 1)
    cases_ = [
        # F_f through Lambda: every robot with a force space, regular ones included (BIE's Lambda is not the identity)
        ("ff_through_lambda", "panda_c3_open", every), ("ff_through_lambda", "planar_4r_force", every),
        # the moment feed-forward under the moment flag: the cell whose force loop is closed and moment loop open
        ("kff_moment_own_flag", "panda_c3_force3", every),
        # r x f dropped: the cells with the offset sensor and a closed moment loop
        ("sensor_no_lever", "panda_c3_closed", every), ("sensor_no_lever", "six_r_mft6_force", every),
        ("integ_after_use", "panda_c3_closed", every), ("integ_after_use", "panda_c3_pi_vsat", every),
        ("integ_after_use", "panda_c4_force", every),
        # a per-component clip: robots with that saturation active
        ("sat_componentwise", "panda_c3_closed", lambda c: d[c]["sat_f"] > 0),
        ("sat_componentwise", "panda_c3_pi_vsat", lambda c: d[c]["sat_w"] > 0),
        ("sat_componentwise", "sliding_base_force", lambda c: d[c]["sat_v"] > 0),
        # 1 / k_v with the zero gain skipped: it changes the norm the linear saturation scales by
        ("vsat_no_pinv", "panda_c3_pi_vsat", lambda c: d[c]["sat_v"] > 0),
        ("type2_from_fu_only", "panda_c3_force3", t2), ("type2_from_fu_only", "panda_c3_open", t2),
        ("goal_wrench_not_rotated", "panda_c3_closed", every), ("goal_wrench_not_rotated", "six_r_mft6_force", every),
    ]
    assert {h for h, _, _ in cases_} == {"ff_through_lambda", "kff_moment_own_flag", "sensor_no_lever", "integ_after_use",
                                         "sat_componentwise", "vsat_no_pinv", "type2_from_fu_only", "goal_wrench_not_rotated"}
    for hook, cell, mask in cases_:
        assert _rejected(cell, d[cell], _pick(mask(cell)), {hook: True}), (hook, cell)
    # and without a hook the same checker accepts the same robots
    assert not _rejected("panda_c3_closed", d["panda_c3_closed"], _pick(every("panda_c3_closed")), {})

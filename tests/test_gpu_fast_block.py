"""The headline kernels read their batch-uniform parameters from the FastBlock of the parameter block (csrc/sai2b_params.h), a
set of copies written at every upload. Hierarchy [full MotionForceTask, full JointTask] on the Panda, three ticks against the
CPU oracle at 1e-10 (torques, and both tasks' integrators at the end), and between the first and the second tick one parameter
the block mirrors is changed through its setter, one case per group of the block:

  entry   gravity compensation on (flags word); both generators on -> off (the law_goals row bases switch back to goals)
  pose    the compliant frame moved and turned
  law     the six gain triples of the MotionForceTask, different on every axis
  chain   MotionForceTask to full dynamic decoupling, the JointTask's bounded-inertia threshold to 0.5
  jt      the JointTask's gains, different on every joint; its velocity saturation off -> on

The tick after the change must be the oracle's with the new value. Batches 1, 63, 64, 65, 130: odd and even sizes (both DMA
branches), a partial last wavefront, a second workgroup. Routes: the one-launch (self) form, the two-launch form, a context made
with SAI2B_NO_BAKED_MODEL=1, a payload on link 3 (tick_fast_payload_kernel<2, *>), and declined robots among regular ones (poses
of tests/singular_poses.py; in a blending region the oracle is met to 1e-6, as everywhere in this suite). The oracle's run of
a case is computed once and shared by the routes."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import payload_cases as pc
import plumbing
import sai2_primitives_perso_amd as pkg
import singular_poses as sp

pytestmark = pytest.mark.gpu
TOL = 1e-10
TICKS = 3
BATCHES = [1, 63, 64, 65, 130]
TASKS = [("mft", {"partial": None}), ("jt", {"selection": None})]
ROUTES = {"self": None, "two_launch": "SAI2B_NO_SELF_SERVE", "no_baked": "SAI2B_NO_BAKED_MODEL"}
WHERE = np.array([0, 63, 64, 100, 129])  # the declined robots of a 130-robot batch: three wavefronts
BANDS = ["inside", "blending", "two", "inside", "blending"]


def _seq(field, start, step=1.0):
    def edit(cfg):
        for i in range(len(field(cfg))):
            field(cfg)[i] = start + step * i
    return edit


def _frame(cfg):
    c, s = np.cos(0.3), np.sin(0.3)
    for i, v in enumerate((0.05, -0.02, 0.1)):
        cfg.frame_pos[i] = v
    for i, v in enumerate((c, -s, 0, s, c, 0, 0, 0, 1)):
        cfg.frame_rot[i] = v


def _mft_gains(cfg):
    for k, (name, v) in enumerate([("kp_pos", 80.0), ("kv_pos", 17.0), ("ki_pos", 2.0), ("kp_ori", 150.0), ("kv_ori", 21.0), ("ki_ori", 3.0)]):
        _seq(lambda c, n=name: getattr(c, n), v, 1.0 + 0.25 * k)(cfg)


def _chain0(cfg):
    cfg.dynamic_decoupling_type = pkg.FULL_DYNAMIC_DECOUPLING


def _chain1(cfg):
    cfg.bie_threshold = 0.5


def _jt_gains(cfg):
    _seq(lambda c: c.kp, 30.0, 2.0)(cfg), _seq(lambda c: c.kv, 9.0, 0.5)(cfg), _seq(lambda c: c.ki, 1.5, 0.25)(cfg)


def _jt_vsat(cfg):
    cfg.use_velocity_saturation = 1
    _seq(lambda c: c.saturation_velocity, 0.05, 0.05)(cfg)  # low enough to bind on some joints, not on all


def _otg(on):
    def edit(cfg):
        cfg.use_internal_otg = int(on)
    return edit


# case: (edits of the configurations at creation, gravity compensation at creation, the change: per-task edits, gravity after)
CASES = {
    "entry_gravity": ((None, None), False, (None, None), True),
    "entry_generators_off": ((_otg(True), _otg(True)), True, (_otg(False), _otg(False)), True),
    "pose_frame": ((None, None), True, (_frame, None), True),
    "law_gains": ((None, None), False, (_mft_gains, None), False),
    "chain_decoupling": ((None, None), True, (_chain0, _chain1), True),
    "jt_gains": ((None, None), False, (None, _jt_gains), False),
    "jt_vsat_on": ((None, None), True, (None, _jt_vsat), True),
}


def _configs(make, case):
    cfgs = make(TASKS)
    for c, ki, first in zip(cfgs, ({"ki_pos": 4.0, "ki_ori": 2.0}, {"ki": 3.0}), CASES[case][0]):
        for k, v in ki.items():
            for i in range(len(getattr(c, k))):
                getattr(c, k)[i] = v
        if first:
            first(c)
    return cfgs


def _inputs(B, declined):
    inp = pkg.workloads.make_inputs(3, B=B, seed=7300 + B)
    if declined:
        arm = np.stack([sp.poses("sliding_base", band, BANDS.count(band), seed=3)[1:, BANDS[:k].count(band)]
                        for k, band in enumerate(BANDS)], axis=1)
        inp["q"] = inp["q"].copy()
        inp["q"][:, WHERE] = arm
    return inp


def _start(c, inp, case):
    if CASES[case][0][0] is not None:  # generators on: they start from the state (as smoke() does)
        c.set_state(inp["q"], inp["dq"])
        c.reinitialize()
    if isinstance(c, pc.PayloadOracles):
        c.load_inputs(inp)
    else:
        ol.load_inputs(c, inp)
    c.enable_gravity_compensation(CASES[case][1])


def _change(c, cfgs, case):
    _, _, edits, gravity = CASES[case]
    for t, edit in enumerate(edits):
        if edit:
            edit(cfgs[t])
            c.update_task_config(t, cfgs[t])
    c.enable_gravity_compensation(gravity)


def _integrators(c):
    if isinstance(c, pkg.Controller):
        return plumbing.integrators(c, TASKS)
    return [c.get_mft_integrators(0), c.get_jt_integrators(1)]


def _run(c, cfgs, inp, case, record_singular=False):
    _start(c, inp, case)
    taus, sing = [], []
    for tick in range(TICKS):
        if tick == 1:
            _change(c, cfgs, case)
        c.update_task_models()
        taus.append(c.compute_control_torques(True))
        if record_singular:
            sing.append(c.get_mft_singularity(0)[2] < 6)
    return taus, sing, _integrators(c)


@functools.lru_cache(maxsize=None)
def _oracle(B, case, payload_link, declined):
    inp = _inputs(B, declined)
    cfgs = _configs(ol.task_configs, case)
    if payload_link is None:
        o = ol.Oracle(ol.panda_model(), cfgs, B, threads=4)
    else:
        o = pc.PayloadOracles(pc.texts("panda", link=payload_link), cfgs, B, threads=2)
    taus, sing, integ = _run(o, cfgs, inp, case, record_singular=declined)
    for a in taus + sing + integ:
        a.setflags(write=False)
    return inp, taus, sing, integ


def _check(B, case, env, monkeypatch, payload_link=None, declined=False):
    inp, taus_o, sing, integ_o = _oracle(B, case, payload_link, declined)
    cfgs = _configs(pkg.task_configs, case)
    if env:
        monkeypatch.setenv(env, "1")
    try:
        g = pkg.Controller(pkg.panda_model(), cfgs, B, introspection=False)
    finally:
        if env:
            monkeypatch.delenv(env)
    if payload_link is not None:
        g.set_link_payload(payload_link, *pc.model_rows("panda", payload_link, *pc.rows(B)))
    _start(g, inp, case)
    for tick in range(TICKS):
        if tick == 1:
            _change(g, cfgs, case)
        g.update_task_models()
        tau = g.compute_control_torques(True)
        e = np.abs(tau - taus_o[tick]).max(axis=0) / np.maximum(np.abs(taus_o[tick]).max(axis=0), 1.0)
        now = sing[tick] if declined else np.zeros(B, dtype=bool)
        reg = e[~now].max() if (~now).any() else 0.0
        print(f"{case} B={B} {env or 'default'} tick {tick}: declined {g.fallback_count()}, torque err {reg:.2e}"
              + (f", in a blending region {e[now].max():.2e}" if now.any() else ""))
        assert reg < TOL, (case, env, tick, int(e.argmax()), e.max())
        if now.any():
            assert e[now].max() < 1e-6, (case, env, tick, e[now].max())
        if declined:
            assert g.fallback_count() >= 1, "some robot was declined"
        else:
            assert g.fallback_count() == 0, "every robot of this workload is the SVD-free kernel's"
    for t, (so, sg) in enumerate(zip(integ_o, _integrators(g))):
        assert np.abs(so).max() > 0, "the integrators moved"
        e = np.abs(sg - so).max(axis=0) / max(np.abs(so).max(), 1e-300)
        if declined:
            e = e[~np.any(sing, axis=0)]
        print(f"{case} B={B} {env or 'default'} task {t}: integrator err {e.max():.2e}")
        assert e.max() < TOL, (case, env, t, int(e.argmax()), e.max())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", list(CASES))
def test_change_between_ticks(case, B, monkeypatch):
    """the one-launch (self) form, every batch size"""
    _check(B, case, None, monkeypatch)


@pytest.mark.parametrize("route", ["two_launch", "no_baked"])
@pytest.mark.parametrize("B", [65, 130])
@pytest.mark.parametrize("case", list(CASES))
def test_change_between_ticks_other_forms(case, B, route, monkeypatch):
    """the two-launch form and the kernels that read the robot constants from the parameter block, odd and even batch"""
    _check(B, case, ROUTES[route], monkeypatch)


@pytest.mark.parametrize("case", list(CASES))
def test_change_between_ticks_payload_on_link_3(case, monkeypatch):
    _check(65, case, None, monkeypatch, payload_link=3)


@pytest.mark.parametrize("route", ["self", "two_launch"])
@pytest.mark.parametrize("case", list(CASES))
def test_change_between_ticks_declined_robots_among_regular_ones(case, route, monkeypatch):
    _check(130, case, ROUTES[route], monkeypatch, declined=True)

"""GPU tests (-m gpu) of the headline tick in one launch (tick_self_kernel<1 | 2, *>, csrc/sai2b_self.hip): the SVD-free body
returns which lanes' robots it declines, and the wavefront runs the lanes-per-robot generic tick for them itself, four robots
per round, in LDS pads that alias the input image. What can go wrong: a declined robot that is served twice, not at all, or
by the wrong group; a fifth robot of a wavefront lost between rounds; a lane past the batch that leaves before the ballot or is
taken for a declined one; pads that overwrite image rows or parked M / g a fast lane still reads; counts the host cannot
trust; and a host that does not leave the form when wavefronts need many rounds, or never comes back.

Panda, [full MotionForceTask] and [full MotionForceTask, full JointTask], the baked model and one read from the parameter
block, four ticks. Declined robots are poses of the singular bands (tests/singular_poses.py). Against the CPU oracle: torques
and both tasks' integrators at 1e-10 (relative, per robot), 1e-6 for robots inside a singularity-blending region, as
tests/test_gpu_fast_one_fk.py. Against the two-launch route (SAI2B_NO_SELF_SERVE=1: tick_fast_kernel and the pass over its
work list), which runs the same per-robot code compiled in other kernels: as many robots declined at every tick, and the
largest relative torque difference, printed, below 1e-12 (differences between builds of this code have been <= 3.3e-15)."""
import numpy as np
import pytest

import cases
import oracle_lib as ol
import plumbing
import sai2_primitives_perso_amd as pkg
import singular_poses as sp

pytestmark = pytest.mark.gpu
TOL, TOL_SINGULAR, TOL_ROUTES = 1e-10, 1e-6, 1e-12
TICKS = 4
GENERIC_ONLY, TWO_LAUNCHES, SELF = 0, 1, 2    # worklist_state()["form"]
HIERARCHIES = {
    "mft": [("mft", {"partial": None})],
    "mft_jt": [("mft", {"partial": None}), ("jt", {"selection": None})],
}
MODELS = ["baked", "modified"]
KI = [{"ki_pos": 4.0, "ki_ori": 2.0}, {"ki": 3.0}]
# (batch, placement): odd-batch DMA (1, 63, 65), a partial last workgroup (63, 65, 130), exactly one (64), lanes past the batch in
# a wavefront that has declined robots (63, 65, 130)
CASES = ([(B, "none") for B in (1, 63, 64, 65, 130)] + [(B, "one") for B in (1, 63, 64, 65, 130)] +
         [(B, "five") for B in (63, 64, 65, 130)] + [(130, "wave0"), (65, "last"), (130, "last"), (65, "nan"), (130, "nan")])


def _where(B, placement):
    """the robots given a singular pose"""
    if placement in ("none", "nan"):
        return np.array([], dtype=int)
    if placement == "one":
        return np.array([B // 2])
    if placement == "five":     # one wavefront, two rounds: groups 0..3 in the first, group 0 again in the second; B = 130: wavefront 1
        return np.array([0, 15, 16, 40, 62]) + (64 if B == 130 else 0)
    if placement == "wave0":
        return np.arange(64)
    return np.array([B - 1])  # "last": alone in its wavefront, every other lane of it past the batch


def _pool():
    """arm poses [7][12] inside the singular band (the slider of that robot dropped, as tests/test_gpu_worklist_counts.py)"""
    return sp.poses("sliding_base", "inside", 12, seed=3)[1:]


def _err(a, ref):
    return np.abs(a - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1.0)


def _state_err(a, ref):
    return np.abs(a - ref).max(axis=0) / max(np.abs(ref).max(), 1e-300)


def _configs(make, hier):
    cfgs = make(HIERARCHIES[hier])
    for t, c in enumerate(cfgs):
        cases.apply_opts(c, KI[t])
        cases.apply_opts(c, {"decoupling": pkg.BOUNDED_INERTIA_ESTIMATES})
    return cfgs


def _model(make, model):
    m = make()
    if model == "modified":     # one link mass away from the compile-time Panda: the host selects the <*, false> kernels
        m.link_mass[1] = 4.2
    return m


def _inputs(hier, B, where):
    inp = pkg.workloads.make_inputs(3 if hier == "mft_jt" else 2, B=B, seed=4100 + B)
    pool = _pool()
    inp["q"] = inp["q"].copy()
    inp["q"][:, where] = pool[:, np.arange(len(where)) % pool.shape[1]]
    return inp


def _controller(hier, model, inp, monkeypatch, self_serve):
    if not self_serve:
        monkeypatch.setenv("SAI2B_NO_SELF_SERVE", "1")
    try:
        g = pkg.Controller(_model(pkg.panda_model, model), _configs(pkg.task_configs, hier), inp["q"].shape[1], introspection=False)
    finally:
        if not self_serve:
            monkeypatch.delenv("SAI2B_NO_SELF_SERVE")
    ol.load_inputs(g, inp)
    g.enable_gravity_compensation(True)
    return g


def _oracle(hier, model, inp):
    o = ol.Oracle(_model(ol.panda_model, model), _configs(ol.task_configs, hier), inp["q"].shape[1], threads=4)
    ol.load_inputs(o, inp)
    o.enable_gravity_compensation(True)
    return o


def _tick(c):
    c.update_task_models()    # the pair runs as one fused tick
    return c.compute_control_torques(True)


def _check_tick(label, o, s, w, skip):
    """one tick of oracle, self route and two-launch route; -> (declined, largest difference between the routes, the two
    routes' torques). skip: mask of robots left out of the comparisons of values (a NaN robot)"""
    tau_o, tau_s, tau_w = _tick(o), _tick(s), _tick(w)
    declined = s.fallback_count()
    assert declined == w.fallback_count(), (label, declined, w.fallback_count())
    now = (o.get_mft_singularity(0)[2] < 6) & ~skip
    reg = ~now & ~skip
    e = _err(tau_s, tau_o)
    d = _err(tau_s[:, ~skip], tau_w[:, ~skip]).max() if (~skip).any() else 0.0
    e_reg, e_sing = (e[reg].max() if reg.any() else 0.0), (e[now].max() if now.any() else 0.0)
    print(f"{label}: declined {declined}, {int(now.sum())} in a blending region, torque err regular {e_reg:.2e} singular {e_sing:.2e}, "
          f"self to two launches {d:.2e}, state {s.worklist_state()}")
    assert e_reg < TOL and e_sing < TOL_SINGULAR, (label, e_reg, e_sing)
    assert d < TOL_ROUTES, (label, d)
    return declined, d, tau_s, tau_w


def _check_integrators(label, hier, o, s, skip):
    tasks = HIERARCHIES[hier]
    for t, (so, sg) in enumerate(zip(plumbing.integrators(o, tasks), plumbing.integrators(s, tasks))):
        assert np.abs(so[:, ~skip]).max() > 0, "the integrators moved"
        e = _state_err(sg[:, ~skip], so[:, ~skip])
        print(f"{label} task {t}: integrator err {e.max():.2e}")
        assert e.max() < TOL, (label, t, int(e.argmax()), e.max())


@pytest.mark.parametrize("B,placement", CASES)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("hier", list(HIERARCHIES))
def test_four_ticks_match_oracle_and_two_launch_route(hier, model, B, placement, monkeypatch):
    where = _where(B, placement)
    inp = _inputs(hier, B, where)
    skip = np.zeros(B, dtype=bool)
    if placement == "nan":    # the certificate fails on a NaN: the robot is declined, and its NaN stays in its own rows
        bad = B - 25
        inp["q"][3, bad] = np.nan
        skip[bad] = True
    o, s, w = _oracle(hier, model, inp), _controller(hier, model, inp, monkeypatch, True), _controller(hier, model, inp, monkeypatch, False)
    label = f"{hier} {model} B={B} {placement}"
    worst = 0.0
    for tick in range(1, TICKS + 1):
        declined, d, tau_s, tau_w = _check_tick(f"{label} tick {tick}", o, s, w, skip)
        worst = max(worst, d)
        # (poses inside the band are singular for the arm alone too, and the certificate declines nothing else of this workload)
        assert declined == len(where) + int(skip.sum()), (label, tick, declined)
        assert s.worklist_state()["form"] == SELF and w.worklist_state()["form"] == TWO_LAUNCHES
        if skip.any():    # the NaN robot itself: NaN exactly where the two-launch route has NaN, and nowhere else
            assert np.isnan(tau_w[:, skip]).any(), "the generic tick should not swallow the NaN"
            assert np.array_equal(np.isnan(tau_s[:, skip]), np.isnan(tau_w[:, skip]))
            assert not np.isnan(tau_s[:, ~skip]).any()
    _check_integrators(label, hier, o, s, skip)
    print(f"{label}: largest self to two-launch torque difference {worst:.2e}")


def test_host_leaves_the_form_for_many_rounds_and_comes_back(monkeypatch):
    """every robot of wavefront 0 of a 130-robot batch is declined from tick 1: sixteen rounds in that wavefront. Before any
    look the form is self; the look of tick 9 (the counts of tick 1: 64 declined, 64 in one wavefront) turns the host to two
    launches; the poses are regular from tick 11 on (declined once more at tick 11, where they leave the singular region and the
    generic tick clears their history), the look of tick 17 still has tick 9's counts, the look of tick 25
    those of tick 17 — nothing declined — and the tick is one launch again. Results within tolerance throughout."""
    hier, model, B = "mft_jt", "baked", 130
    where = _where(B, "wave0")
    singular, regular = _inputs(hier, B, where), _inputs(hier, B, where[:0])
    o, s, w = _oracle(hier, model, singular), _controller(hier, model, singular, monkeypatch, True), _controller(hier, model, singular, monkeypatch, False)
    skip = np.zeros(B, dtype=bool)
    for tick in range(1, 27):
        inp = singular if tick <= 10 else regular
        for c in (o, s, w):
            c.set_state(inp["q"], inp["dq"])
        declined = _check_tick(f"B={B} tick {tick}", o, s, w, skip)[0]
        # (tick 11: regular again, but a robot that leaves a singular region is the generic tick's once more, which clears its history)
        assert declined == (64 if tick <= 11 else 0), (tick, declined)
        state = s.worklist_state()
        want_seen = -1 if tick < 9 else (64 if tick < 25 else 0)
        want_form = SELF if tick < 9 or tick >= 25 else TWO_LAUNCHES
        assert state["last_seen"] == want_seen and state["wmax"] == want_seen, (tick, state)
        assert state["form"] == want_form, (tick, state)
        assert w.worklist_state()["form"] == TWO_LAUNCHES, tick
    _check_integrators(f"B={B}", hier, o, s, skip)

"""GPU tests (-m gpu) of the baked kernels' model phase written out from the Panda's nonzero terms
(csrc/tools/gen_baked_model.cpp -> sai2b_baked_panda_model.h): tick_fast_kernel<1 | 2, true> and the payload forms take
fk / jacobian / mass_matrix / gravity_vector from it. What can go wrong is a dropped term that was not zero, a sum in
another order than rounding allows, a frame entry read as the constant it is only for another link, and a NaN that no
longer travels where the generic product with an exact zero carried it.

Panda [full MotionForceTask] and [full MotionForceTask, full JointTask] through the ordinary Controller, 3 consecutive
ticks, against the CPU oracle: torques of every tick and the integrators of every task after the last one at the 1e-10
(relative, per robot) of tests/test_gpu_fast_one_fk.py, 1e-6 inside singularity-blending regions as there. The same
inputs run through a context made with SAI2B_NO_BAKED_MODEL=1 (the generic functions on the parameter block): it must
decline as many robots every tick (the work list itself is not readable from outside; a robot is declined from J and
its own state alone), and the largest baked-to-generic difference is printed."""
import numpy as np
import pytest

import cases
import oracle_lib as ol
import payload_cases as pc
import plumbing
import sai2_primitives_perso_amd as pkg
import singular_poses as sp

pytestmark = pytest.mark.gpu
TOL = 1e-10
TICKS = 3
BATCHES = [1, 63, 64, 65, 130]  # odd-batch DMA, a partial workgroup, exactly one, two workgroups
HIERARCHIES = {
    "mft": [("mft", {"partial": None})],
    "mft_jt": [("mft", {"partial": None}), ("jt", {"selection": None})],
}
KI = [{"ki_pos": 4.0, "ki_ori": 2.0}, {"ki": 3.0}]
VSAT = [{"velocity_saturation": (0.05, 0.1)}, {"velocity_saturation": 0.2}]
BIE, FULL, IMP = pkg.BOUNDED_INERTIA_ESTIMATES, pkg.FULL_DYNAMIC_DECOUPLING, pkg.IMPEDANCE
# name: decoupling of both tasks, velocity saturation, with_comp, gravity compensation (g and both uses of M)
VARIANTS = {
    "bie_bie": (BIE, False, True, False),
    "full_full_vsat_nocomp_gravity": (FULL, True, False, True),
    "imp_imp_gravity": (IMP, False, True, True),
}


def _err(a, ref):
    return np.abs(a - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1.0)


def _state_err(a, ref):
    return np.abs(a - ref).max(axis=0) / max(np.abs(ref).max(), 1e-300)


def _configs(make, tasks, variant):
    dec, vsat, _, _ = VARIANTS[variant]
    cfgs = make(tasks)
    for t, c in enumerate(cfgs):
        cases.apply_opts(c, KI[t])
        cases.apply_opts(c, {"decoupling": dec})
        if vsat:
            cases.apply_opts(c, VSAT[t])
    return cfgs


def _inputs(hier, B, q=None):
    inp = pkg.workloads.make_inputs(3 if hier == "mft_jt" else 2, B=B, seed=700 + B)
    if q is not None:
        inp["q"] = q(inp["q"])
    return inp


def _controller(hier, variant, inp, monkeypatch, baked=True, payload_link=None):
    """the GPU side; baked=False: the same context with the model read from the parameter block"""
    B = inp["q"].shape[1]
    if not baked:
        monkeypatch.setenv("SAI2B_NO_BAKED_MODEL", "1")
    try:
        g = pkg.Controller(pkg.panda_model(), _configs(pkg.task_configs, HIERARCHIES[hier], variant), B, introspection=False)
    finally:
        if not baked:
            monkeypatch.delenv("SAI2B_NO_BAKED_MODEL")
    ol.load_inputs(g, inp)
    g.enable_gravity_compensation(VARIANTS[variant][3])
    if payload_link is not None:
        g.set_link_payload(payload_link, *pc.model_rows("panda", payload_link, *pc.rows(B)))
    return g


def _oracle(hier, variant, inp, payload_link=None):
    B = inp["q"].shape[1]
    cfgs = _configs(ol.task_configs, HIERARCHIES[hier], variant)
    if payload_link is None:
        o = ol.Oracle(ol.panda_model(), cfgs, B, threads=4)
        ol.load_inputs(o, inp)
    else:
        o = pc.PayloadOracles(pc.texts("panda", link=payload_link), cfgs, B, threads=2)
        o.load_inputs(inp)
    o.enable_gravity_compensation(VARIANTS[variant][3])
    return o


def _tick(c, with_comp):
    c.update_task_models()
    return c.compute_control_torques(with_comp)


def _integrators(c, tasks):
    if isinstance(c, pkg.Controller):
        return plumbing.integrators(c, tasks)
    return [c.get_mft_integrators(t) if kind == "mft" else c.get_jt_integrators(t) for t, (kind, _) in enumerate(tasks)]


def _run(hier, variant, inp, monkeypatch, payload_link=None, singular=None):
    """3 ticks of oracle, baked and generic contexts on the same inputs; singular(o) -> mask of the robots held to 1e-6"""
    tasks, with_comp = HIERARCHIES[hier], VARIANTS[variant][2]
    o = _oracle(hier, variant, inp, payload_link)
    g = _controller(hier, variant, inp, monkeypatch, True, payload_link)
    n = _controller(hier, variant, inp, monkeypatch, False, payload_link)
    B, worst = g.B, 0.0
    loose = np.zeros(B, dtype=bool)
    counts = []
    for tick in range(TICKS):
        tau_o, tau_g, tau_n = _tick(o, with_comp), _tick(g, with_comp), _tick(n, with_comp)
        assert g.fallback_count() == n.fallback_count(), (tick, g.fallback_count(), n.fallback_count())
        counts.append(g.fallback_count())
        now = singular(o) if singular else np.zeros(B, dtype=bool)
        loose |= now
        e, d = _err(tau_g, tau_o), _err(tau_g, tau_n)
        worst = max(worst, d[~now].max() if (~now).any() else 0.0)
        print(f"{hier} {variant} B={B} tick {tick}: declined {counts[-1]}, torque err {e[~now].max():.2e}, baked to generic {d.max():.2e}")
        assert e[~now].max() < TOL, (tick, int(e.argmax()), e.max())
        if now.any():
            assert e[now].max() < 1e-6, (tick, e[now].max())
    for t, (so, sg) in enumerate(zip(_integrators(o, tasks), _integrators(g, tasks))):
        assert np.abs(so).max() > 0, "the integrators moved"
        e = _state_err(sg, so)
        print(f"{hier} {variant} B={B} task {t}: integrator err {e.max():.2e}")
        assert e.max() < TOL, (t, int(e.argmax()), e.max())
    print(f"{hier} {variant} B={B}: largest baked-to-generic torque difference {worst:.2e}")
    # two routes of one law at 1e-10 of the oracle each; far closer in fact (rounding of the model phase only)
    assert worst < 2 * TOL
    return counts


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("hier", list(HIERARCHIES))
def test_three_ticks_match_oracle_and_generic_route(hier, variant, B, monkeypatch):
    counts = _run(hier, variant, _inputs(hier, B), monkeypatch)
    assert counts == [0] * TICKS, "every robot of this workload is the SVD-free kernel's"


@pytest.mark.parametrize("hier", list(HIERARCHIES))
def test_declined_robots_among_regular_ones(hier, monkeypatch):
    """poses of the singular bands (tests/singular_poses.py) in three wavefronts of a 130-robot batch: both routes decline
    them from the same Jacobian test, and their neighbours stay at 1e-10"""
    B = 130
    where = np.array([0, 63, 64, 100, 129])
    bands = ["inside", "blending", "two", "inside", "blending"]
    arm = np.stack([sp.poses("sliding_base", band, bands.count(band), seed=3)[1:, bands[:k].count(band)]
                    for k, band in enumerate(bands)], axis=1)

    def put(q):
        q = q.copy()
        q[:, where] = arm
        return q

    def singular(o):
        s = o.get_mft_singularity(0)[2] < 6
        assert not s[np.setdiff1d(np.arange(B), where)].any()
        return s

    counts = _run(hier, "bie_bie", _inputs(hier, B, q=put), monkeypatch, singular=singular)
    assert all(3 <= c <= len(where) for c in counts), counts


@pytest.mark.parametrize("hier", list(HIERARCHIES))
def test_payload_on_link_3(hier, monkeypatch):
    """tick_fast_payload_kernel<*, true>: the composite-body loops written out, with the payload's terms added at link 3 by
    the selects of the generic form; robot b carries payload b % 16 (tests/payload_cases.py), one oracle per payload"""
    counts = _run(hier, "full_full_vsat_nocomp_gravity", _inputs(hier, 65), monkeypatch, payload_link=3)
    assert counts == [0] * TICKS


def test_nan_in_one_robot_stays_in_that_robot(monkeypatch):
    """One q entry of robot 40 of 65 is NaN. The generic functions multiply it by the model's exact zeros, the written-out
    ones do not: its torques must be NaN on the baked route exactly where the generic route has NaN, and every other
    robot's torques are bit-equal to a run in which robot 40 is an ordinary robot."""
    hier, variant, B, bad = "mft_jt", "imp_imp_gravity", 65, 40
    with_comp = VARIANTS[variant][2]

    def put(q):
        q = q.copy()
        q[3, bad] = np.nan
        return q

    clean, dirty = _inputs(hier, B), _inputs(hier, B, q=put)
    ref = _controller(hier, variant, clean, monkeypatch)
    g = _controller(hier, variant, dirty, monkeypatch)
    n = _controller(hier, variant, dirty, monkeypatch, baked=False)
    others = np.arange(B) != bad
    for tick in range(TICKS):
        tau_r, tau_g, tau_n = _tick(ref, with_comp), _tick(g, with_comp), _tick(n, with_comp)
        assert g.fallback_count() == n.fallback_count()
        print(f"tick {tick}: declined {g.fallback_count()}, NaN torques baked {np.isnan(tau_g[:, bad]).sum()} generic {np.isnan(tau_n[:, bad]).sum()}")
        assert np.isnan(tau_n[:, bad]).any(), "the generic route should not swallow the NaN"
        assert np.array_equal(np.isnan(tau_g[:, bad]), np.isnan(tau_n[:, bad]))
        assert np.array_equal(tau_g[:, others], tau_r[:, others])

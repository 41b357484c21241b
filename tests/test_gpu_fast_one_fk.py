"""GPU tests (-m gpu) of the headline tick's one-FK form: tick_fast_kernel<2, *> runs CRBA and gravity inside its DMA
window, parks M and g in LDS, and evaluates the JointTask law (and stores its integrators) behind the nullspace vector
from plain loads. What can go wrong is a row that reaches the wrong robot (odd-batch DMA, clamped columns of a partial
workgroup, the parked column of another lane), a JointTask integrator stored twice or not at all, and a declined robot
whose state the fast kernel touched before the work-list pass.

The [full MotionForceTask, full JointTask] hierarchy on the Panda through the ordinary Controller, 3 consecutive ticks,
against the CPU oracle: torques of every tick and the integrator state of both tasks after the last one, at the 1e-10
(relative, per robot) of tests/test_gpu_parity.py. Robots inside a singularity-blending region invert a nearly singular
matrix and are held to 1e-6 there, as in that file."""
import numpy as np
import pytest

import cases
import oracle_lib as ol
import plumbing
import sai2_primitives_perso_amd as pkg
import singular_poses as sp

pytestmark = pytest.mark.gpu
N = pkg.DOF
TOL = 1e-10
TICKS = 3
# the odd-batch 4-byte DMA (1, 63, 65, 127), the even path with a partial last workgroup (130), clamped columns (all but
# 64), more than one workgroup (65, 127, 130)
BATCHES = [1, 63, 64, 65, 127, 130]
TASKS = [("mft", {"partial": None}), ("jt", {"selection": None})]
KI = [{"ki_pos": 4.0, "ki_ori": 2.0}, {"ki": 3.0}]  # a JointTask integrator stored twice or not at all shows in the torques
VSAT = [{"velocity_saturation": (0.05, 0.1)}, {"velocity_saturation": 0.2}]
BIE, FULL, IMP = pkg.BOUNDED_INERTIA_ESTIMATES, pkg.FULL_DYNAMIC_DECOUPLING, pkg.IMPEDANCE
# name: decoupling of the MotionForceTask, of the JointTask, velocity saturation, with_comp, gravity compensation
VARIANTS = {
    "bie_bie": (BIE, BIE, False, True, False),
    "full_full_vsat_nocomp_gravity": (FULL, FULL, True, False, True),
    "imp_imp_gravity": (IMP, IMP, False, True, True),
    "full_bie_vsat_nocomp": (FULL, BIE, True, False, False),
    "bie_imp_vsat_gravity": (BIE, IMP, True, True, True),
}


def _err(a, ref):
    return np.abs(a - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1.0)


def _state_err(a, ref):
    """integrators are small numbers (an error times dt per tick): relative to the largest of the row set, per robot"""
    return np.abs(a - ref).max(axis=0) / max(np.abs(ref).max(), 1e-300)


def _pair(variant, B, models=None, q=None, seed=0):
    d0, d1, vsat, with_comp, gravity = VARIANTS[variant]
    inp = pkg.workloads.make_inputs(3, B=B, seed=900 + B + seed)
    if q is not None:
        inp["q"] = q(inp["q"])
    go, gg = ol.task_configs(TASKS), pkg.task_configs(TASKS)
    for cfgs in (go, gg):
        for t, c in enumerate(cfgs):
            cases.apply_opts(c, KI[t])
            cases.apply_opts(c, {"decoupling": (d0, d1)[t]})
            if vsat:
                cases.apply_opts(c, VSAT[t])
    mo, mg = models if models else (ol.panda_model(), pkg.panda_model())
    o = ol.Oracle(mo, go, B, threads=4)
    g = pkg.Controller(mg, gg, B, introspection=False)
    for c in (o, g):
        ol.load_inputs(c, inp)
        c.enable_gravity_compensation(gravity)
    return o, g, with_comp


def _tick(c, with_comp):
    c.update_task_models()  # the pair runs as one fused tick (test_split_calls_run_the_fused_tick_and_flush_when_observed)
    return c.compute_control_torques(with_comp)


def _run_regular(o, g, with_comp):
    B = g.B
    for tick in range(TICKS):
        tau_o, tau_g = _tick(o, with_comp), _tick(g, with_comp)
        assert g.fallback_count() == 0, "every robot of this workload is the SVD-free kernel's"
        e = _err(tau_g, tau_o)
        print(f"B={B} tick {tick}: torque err {e.max():.2e}")
        assert e.max() < TOL, (tick, int(e.argmax()), e.max())
    for t, (so, sg) in enumerate(zip(plumbing.integrators(o, TASKS), plumbing.integrators(g, TASKS))):
        assert np.abs(so).max() > 0, "the integrators moved"
        e = _state_err(sg, so)
        print(f"B={B} task {t}: integrator err {e.max():.2e}")
        assert e.max() < TOL, (t, int(e.argmax()), e.max())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_three_ticks_match_oracle(variant, B):
    _run_regular(*_pair(variant, B))


@pytest.mark.parametrize("B", [65, 130])
def test_model_from_the_parameter_block(B):
    """one link mass away from the compile-time Panda: the host selects tick_fast_kernel<2, false>"""
    mo, mg = ol.panda_model(), pkg.panda_model()
    for m in (mo, mg):
        m.link_mass[1] = 4.2
    _run_regular(*_pair("bie_imp_vsat_gravity", B, models=(mo, mg)))
    mo, mg = ol.panda_model(), pkg.panda_model()
    for m in (mo, mg):
        m.link_mass[1] = 4.2
    _run_regular(*_pair("full_full_vsat_nocomp_gravity", B, models=(mo, mg)))


def test_declined_robots_among_regular_ones():
    """Poses of the singular bands (tests/singular_poses.py, the arm joints of its Panda on a slider) in three
    wavefronts of a 130-robot batch. The fast kernel declines them before it touches any state; the generic pass behind
    it takes them from the work list. Their neighbours in the same wavefronts stay at 1e-10, and nobody's integrators
    advance twice."""
    B = 130
    where = np.array([0, 63, 64, 100, 129])
    bands = ["inside", "blending", "two", "inside", "blending"]
    arm = np.stack([sp.poses("sliding_base", band, bands.count(band), seed=3)[1:, bands[:k].count(band)]
                    for k, band in enumerate(bands)], axis=1)

    def put(q):
        q = q.copy()
        q[:, where] = arm
        return q

    o, g, with_comp = _pair("bie_bie", B, q=put)
    singular_seen = np.zeros(B, dtype=bool)
    for tick in range(TICKS):
        tau_o, tau_g = _tick(o, with_comp), _tick(g, with_comp)
        _, _, ro = o.get_mft_singularity(0)
        singular = ro < 6
        singular_seen |= singular
        assert not singular[np.setdiff1d(np.arange(B), where)].any()
        assert singular[where].sum() >= 3, "the borrowed poses should be singular for the arm alone too"
        # the certificate is conservative: it may also decline a regular robot among the ones placed
        assert singular.sum() <= g.fallback_count() <= len(where)
        e = _err(tau_g, tau_o)
        print(f"tick {tick}: {singular.sum()} singular, {g.fallback_count()} declined, err regular {e[~singular].max():.2e} "
              f"singular {e[singular].max():.2e}")
        assert e[~singular].max() < TOL, (tick, e[~singular].max())
        assert e[singular].max() < 1e-6, (tick, e[singular].max())
    for t, (so, sg) in enumerate(zip(plumbing.integrators(o, TASKS), plumbing.integrators(g, TASKS))):
        e = _state_err(sg, so)
        print(f"task {t}: integrator err regular {e[~singular_seen].max():.2e} singular {e[singular_seen].max():.2e}")
        assert e.max() < TOL, (t, int(e.argmax()), e.max())  # (the laws' integrators do not see the singularity)

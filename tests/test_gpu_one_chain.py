"""GPU tests (-m gpu) of the two-level fast tick's one-chain form (csrc/sai2b_chain.h through fast_tick<true>:
tick_fast_kernel<2, *>, tick_self_kernel<2, *>, tick_fast_payload_kernel<2, *>): one whitened chain on Mb or M, Householder
QR instead of Gram matrix + Cholesky + pivot search, the MotionForceTask torques recovered through the chain, the nullspace
pair from nv = Lx^-T Q e_6 and M nv, and at most one further Cholesky behind a batch-uniform branch. What can go wrong
is a branch of the decoupling combinations that picks the wrong factor (a^T M^-1 tau_mft wants M's, beta wants Mb's), a
threshold that raises no / some / every diagonal element, a batch whose last wavefront is partial, and the [MFT] kernels,
which keep their Gram + Cholesky form, drifting with the shared code.

Panda through the ordinary Controller, 3 consecutive ticks, against the CPU oracle: torques of every tick and the
integrators of every task after the last one at 1e-10 (relative, per robot), 1e-6 for robots inside a singularity-blending
region, as in tests/test_gpu_baked_structure.py. Every case also runs a context made with SAI2B_NO_BAKED_MODEL=1 (the
<*, false> kernels), held to the same bound."""
import itertools

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
BATCHES = [1, 63, 64, 65, 130]  # odd-batch DMA, a partial workgroup, exactly one, one and a lane, two and two lanes
THRESHOLDS = [0.0, 0.1, 0.5, 5.0]  # no, one, several, every diagonal element of the Panda's M raised
HIERARCHIES = {
    "mft": [("mft", {"partial": None})],
    "mft_jt": [("mft", {"partial": None}), ("jt", {"selection": None})],
}
KI = [{"ki_pos": 4.0, "ki_ori": 2.0}, {"ki": 3.0}]
DEC = {"bie": pkg.BOUNDED_INERTIA_ESTIMATES, "full": pkg.FULL_DYNAMIC_DECOUPLING, "imp": pkg.IMPEDANCE}


def _err(a, ref):
    return np.abs(a - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1.0)


def _state_err(a, ref):
    return np.abs(a - ref).max(axis=0) / max(np.abs(ref).max(), 1e-300)


def _configs(make, hier, decs, thr):
    cfgs = make(HIERARCHIES[hier])
    for t, c in enumerate(cfgs):
        cases.apply_opts(c, KI[t])
        cases.apply_opts(c, {"decoupling": DEC[decs[t]], "bie_threshold": thr})
    return cfgs


def _inputs(hier, B, q=None):
    inp = pkg.workloads.make_inputs(3 if hier == "mft_jt" else 2, B=B, seed=5200 + B)
    if q is not None:
        inp["q"] = q(inp["q"])
    return inp


def _controller(hier, decs, thr, gravity, inp, monkeypatch, env=None, payload_link=None):
    B = inp["q"].shape[1]
    if env:
        monkeypatch.setenv(env, "1")
    try:
        g = pkg.Controller(pkg.panda_model(), _configs(pkg.task_configs, hier, decs, thr), B, introspection=False)
    finally:
        if env:
            monkeypatch.delenv(env)
    ol.load_inputs(g, inp)
    g.enable_gravity_compensation(gravity)
    if payload_link is not None:
        g.set_link_payload(payload_link, *pc.model_rows("panda", payload_link, *pc.rows(B)))
    return g


def _oracle(hier, decs, thr, gravity, inp, payload_link=None):
    B = inp["q"].shape[1]
    cfgs = _configs(ol.task_configs, hier, decs, thr)
    if payload_link is None:
        o = ol.Oracle(ol.panda_model(), cfgs, B, threads=4)
        ol.load_inputs(o, inp)
    else:
        o = pc.PayloadOracles(pc.texts("panda", link=payload_link), cfgs, B, threads=2)
        o.load_inputs(inp)
    o.enable_gravity_compensation(gravity)
    return o


def _tick(c, with_comp):
    c.update_task_models()
    return c.compute_control_torques(with_comp)


def _integrators(c, tasks):
    if isinstance(c, pkg.Controller):
        return plumbing.integrators(c, tasks)
    return [c.get_mft_integrators(t) if kind == "mft" else c.get_jt_integrators(t) for t, (kind, _) in enumerate(tasks)]


def _run(label, hier, decs, thr, with_comp, gravity, inp, monkeypatch, routes=(None, "SAI2B_NO_BAKED_MODEL"), payload_link=None,
         singular=None):
    """3 ticks of the oracle and of one context per route (an environment switch at creation, or None) on the same
    inputs; singular(o) -> mask of the robots held to 1e-6. Returns the declined counts per tick of the first route."""
    tasks = HIERARCHIES[hier]
    o = _oracle(hier, decs, thr, gravity, inp, payload_link)
    gs = [_controller(hier, decs, thr, gravity, inp, monkeypatch, env, payload_link) for env in routes]
    B, counts = inp["q"].shape[1], []
    for tick in range(TICKS):
        tau_o = _tick(o, with_comp)
        now = singular(o) if singular else np.zeros(B, dtype=bool)
        for env, g in zip(routes, gs):
            e = _err(_tick(g, with_comp), tau_o)
            assert g.fallback_count() == gs[0].fallback_count(), (label, env, tick)
            reg = e[~now].max() if (~now).any() else 0.0
            print(f"{label} B={B} {env or 'default'} tick {tick}: declined {g.fallback_count()}, torque err {reg:.2e}"
                  + (f", in a blending region {e[now].max():.2e}" if now.any() else ""))
            assert reg < TOL, (label, env, tick, int(e.argmax()), e.max())
            if now.any():
                assert e[now].max() < 1e-6, (label, env, tick, e[now].max())
        counts.append(gs[0].fallback_count())
    so_all = _integrators(o, tasks)
    for env, g in zip(routes, gs):
        for t, (so, sg) in enumerate(zip(so_all, _integrators(g, tasks))):
            assert np.abs(so).max() > 0, "the integrators moved"
            e = _state_err(sg, so)
            print(f"{label} B={B} {env or 'default'} task {t}: integrator err {e.max():.2e}")
            assert e.max() < TOL, (label, env, t, int(e.argmax()), e.max())
    return counts


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("hier", list(HIERARCHIES))
def test_batches(hier, B, monkeypatch):
    """the library's default configuration (both tasks bounded-inertia at 0.1, with_comp): chain on Mb, Cholesky of M
    for the compensation"""
    counts = _run(f"{hier} bie/bie", hier, ("bie", "bie"), 0.1, True, B % 2 == 0, _inputs(hier, B), monkeypatch)
    assert counts == [0] * TICKS, "every robot of this workload is the SVD-free kernel's"


COMBOS = list(itertools.product(DEC, DEC, (False, True)))


@pytest.mark.parametrize("k", range(len(COMBOS)), ids=[f"{m}_{j}_{'comp' if c else 'nocomp'}" for m, j, c in COMBOS])
def test_decoupling_combinations(k, monkeypatch):
    """3 x 3 decouplings x with_comp: which matrix the chain runs on, whether a second factor is taken and of which
    matrix. The threshold walks through all four and gravity compensation alternates along the way."""
    mft, jt, comp = COMBOS[k]
    thr, gravity = THRESHOLDS[k % 4], (k // 2) % 2 == 0
    counts = _run(f"{mft}/{jt} thr {thr} comp {comp} gravity {gravity}", "mft_jt", (mft, jt), thr, comp, gravity,
                  _inputs("mft_jt", 65), monkeypatch)
    assert counts == [0] * TICKS


@pytest.mark.parametrize("comp", [False, True])
@pytest.mark.parametrize("gravity", [False, True])
@pytest.mark.parametrize("thr", THRESHOLDS)
def test_thresholds(thr, gravity, comp, monkeypatch):
    """bounded inertia on both tasks with none, one, several and all diagonal elements raised"""
    counts = _run(f"bie/bie thr {thr} comp {comp} gravity {gravity}", "mft_jt", ("bie", "bie"), thr, comp, gravity,
                  _inputs("mft_jt", 64), monkeypatch)
    assert counts == [0] * TICKS


@pytest.mark.parametrize("decs", [("bie", "bie"), ("full", "bie")])
@pytest.mark.parametrize("hier", list(HIERARCHIES))
def test_declined_robots_among_regular_ones(hier, decs, monkeypatch):
    """poses of the singular bands (tests/singular_poses.py) in three wavefronts of a 130-robot batch, through the
    one-launch form (each wavefront serves the robots it declines) and the two-launch form (SAI2B_NO_SELF_SERVE=1: the
    generic pass over the work list): the declined robots take the generic tick, their neighbours stay at 1e-10"""
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

    counts = _run(f"{hier} {'/'.join(decs)} declined", hier, decs, 0.1, True, True, _inputs(hier, B, q=put), monkeypatch,
                  routes=(None, "SAI2B_NO_SELF_SERVE", "SAI2B_NO_BAKED_MODEL"), singular=singular)
    assert all(3 <= c <= len(where) for c in counts), counts


@pytest.mark.parametrize("decs,comp", [(("bie", "bie"), True), (("full", "bie"), True), (("imp", "full"), False)])
def test_payload_on_link_3(decs, comp, monkeypatch):
    """tick_fast_payload_kernel<2, *>: M arrives as an array, not from the parked rows, and the JointTask law is given
    early; robot b carries payload b % 16 (tests/payload_cases.py), one oracle per payload"""
    counts = _run(f"payload {'/'.join(decs)}", "mft_jt", decs, 0.5, comp, True, _inputs("mft_jt", 65), monkeypatch, payload_link=3)
    assert counts == [0] * TICKS

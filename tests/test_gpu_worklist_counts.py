"""GPU tests (-m gpu) of how the length of the tick's work list reaches the host: the pass over the list (tick_group_kernel)
writes two tagged 8-byte words into mapped host memory when the host asks, in place of two copy kernels and an event behind
it. What can go wrong: a count the host acts on that is not the one of eight ticks before (a stale or a neighbouring tick's
words, a torn pair), a request that is never answered, and a result that changes with the way the counts travel.

The [full MotionForceTask, full JointTask] hierarchy on the Panda, 20 ticks, the list one robot longer at each of the first
twelve (poses of the singular bands, tests/singular_poses.py). The route through the words (the default) against the route
that keeps the copies (SAI2B_GENERIC_LANES=1: the one-lane generic kernel as the pass, which does not take the pointer) and
against the CPU oracle: torques at 1e-10 (relative, per robot; robots inside a singularity-blending region at 1e-6, as
tests/test_gpu_fast_one_fk.py), integrators at 1e-10."""
import numpy as np
import pytest

import cases
import oracle_lib as ol
import plumbing
import sai2_primitives_perso_amd as pkg
import singular_poses as sp

pytestmark = pytest.mark.gpu
TOL = 1e-10
TASKS = [("mft", {"partial": None}), ("jt", {"selection": None})]
KI = [{"ki_pos": 4.0, "ki_ori": 2.0}, {"ki": 3.0}]
WORDS, COPIES = 1, 2  # sai2b_get_worklist_state: how the request under way is answered


def _err(a, ref):
    return np.abs(a - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1.0)


def _configs(make):
    cfgs = make(TASKS)
    for t, c in enumerate(cfgs):
        cases.apply_opts(c, KI[t])
        cases.apply_opts(c, {"decoupling": pkg.BOUNDED_INERTIA_ESTIMATES})
    return cfgs


def _controller(inp, monkeypatch, one_lane_pass):
    if one_lane_pass:
        monkeypatch.setenv("SAI2B_GENERIC_LANES", "1")
    try:
        g = pkg.Controller(pkg.panda_model(), _configs(pkg.task_configs), inp["q"].shape[1], introspection=False)
    finally:
        if one_lane_pass:
            monkeypatch.delenv("SAI2B_GENERIC_LANES")
    ol.load_inputs(g, inp)
    return g


def _tick(c):
    c.update_task_models()
    return c.compute_control_torques(True)


def test_host_acts_on_the_counts_of_eight_ticks_before(monkeypatch):
    """what the host last saw is, from tick 9 on, the count of tick 1 and, from tick 17 on, that of tick 9 — neither the
    current one nor a neighbour's — whichever way the counts travel"""
    B = 130
    inp = pkg.workloads.make_inputs(3, B=B, seed=1300 + B)
    pool = sp.poses("sliding_base", "inside", 12, seed=3)[1:]
    o = ol.Oracle(ol.panda_model(), _configs(ol.task_configs), B, threads=4)
    ol.load_inputs(o, inp)
    w, c = _controller(inp, monkeypatch, False), _controller(inp, monkeypatch, True)
    length = lambda tick: min(tick, 12)  # ticks count from 1
    counts = {}
    for tick in range(1, 21):
        q = inp["q"].copy()
        q[:, :length(tick)] = pool[:, :length(tick)]
        for x in (o, w, c):
            x.set_state(q, inp["dq"])
        tau_o, tau_w, tau_c = _tick(o), _tick(w), _tick(c)
        counts[tick] = w.fallback_count()
        assert counts[tick] == c.fallback_count(), tick
        now = o.get_mft_singularity(0)[2] < 6
        e, d = _err(tau_w, tau_o), _err(tau_w, tau_c)
        reg, sing = (e[~now].max() if (~now).any() else 0.0), (e[now].max() if now.any() else 0.0)
        print(f"B={B} tick {tick}: declined {counts[tick]}, host saw {w.worklist_state()['last_seen']}, torque err regular {reg:.2e} "
              f"singular {sing:.2e}, words to copies {d.max():.2e}")
        assert reg < TOL and sing < 1e-6, tick
        want = -1 if tick < 9 else (counts[1] if tick < 17 else counts[9])
        for name, x, kind in (("words", w, WORDS), ("copies", c, COPIES)):
            state = x.worklist_state()
            assert state["last_seen"] == want, (name, tick, state, counts)
            assert state["pending"] == kind, (name, tick, state)  # (a request is always under way: asked at ticks 1, 9, 17)
    print(f"B={B}: declined per tick {counts}")
    # (a neighbouring tick's count, or the current one, would show)
    assert counts[1] != counts[2] and counts[9] not in (counts[8], counts[10], counts[17]), counts
    for t, (so, sg) in enumerate(zip(plumbing.integrators(o, TASKS), plumbing.integrators(w, TASKS))):
        e = np.abs(sg - so).max(axis=0) / max(np.abs(so).max(), 1e-300)
        print(f"B={B} task {t}: integrator err {e.max():.2e}")
        assert e.max() < TOL, (t, int(e.argmax()), e.max())

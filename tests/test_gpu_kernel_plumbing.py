"""Every per-robot input row reaches its robot in the tick kernels of the Panda hierarchies (-m gpu).

The inputs (tests/plumbing.py) make every row a kernel reads visible: JointTask goals dq and ddq, goal and sensed
wrench, integral gains on every task, robots leaving a singular region. Routes, each forced before the ctx is made:
  c2            [full MFT]                  tick_fast_kernel<1, true>  (inputs in registers)
  c3            [full MFT, full JT]         tick_fast_kernel<2, true>  (inputs staged in LDS by DMA)
  c3_model      the same, modified arm      tick_fast_kernel<2, false>
  c4            [MFT pos, JT 2 joints, JT]  tick_cert_kernel<3>
  c3_sing6      SAI2B_FORCE_SING6           tick_cert_kernel<6, S6>
  c3_introspect introspection on            tick_kernel<true> (the generic kernel)
(a) parity with the oracle at ragged batch sizes, torques, integrators (read back from the device), singularity
bookkeeping and the work list's length every tick; (b) one robot per input row perturbed: the others stay
bit-identical, the perturbed ones follow the oracle; (c) a robot's results do not depend on where it sits in the
batch; (d) C5's 524 288 robots in one ctx and in eight.
"""
import numpy as np
import pytest

import oracle_lib as ol
import plumbing as pl
import sai2_primitives_perso_amd as pkg
from plumbing import WARMUP

pytestmark = pytest.mark.gpu
N = pkg.DOF
TOL, TOL_SINGULAR, TOL_INTEG = 1e-10, 1e-6, 1e-12
MEASURED = 6
# config, force space, modified arm, introspection, environment
ROUTES = {
    "c2": (2, True, False, False, {}),
    "c3": (3, True, False, False, {}),
    "c3_model": (3, True, True, False, {}),
    "c4": (4, False, False, False, {}),
    "c3_sing6": (3, True, False, False, {"SAI2B_FORCE_SING6": "1"}),
    "c3_introspect": (3, True, False, True, {}),
}
FAST = ("c2", "c3", "c3_model")  # the SVD-free kernels: no in-lane singular branch, every declined robot is listed
BATCHES = (1, 2, 3, 31, 33, 62, 63, 64, 65, 66, 127, 129, 4097)
BIG = (65535, 65538)
# certified by tick_fast_kernel above s_max * 6^(1/16) = 0.0671 (sai2b_fast.hpp); below, a regular robot may be declined
GREY = 0.075


def _err(tau, ref):
    return np.abs(tau - ref).max(axis=0) / np.maximum(np.abs(ref).max(axis=0), 1.0)


def _make(route, inp, monkeypatch, threads=8):
    config, force, modified, introspection, env = ROUTES[route]
    co, cg = pl.configs(inp.tasks, force)
    mo, mg = ol.panda_model(), pkg.panda_model()
    if modified:
        pl.modified_model(mo), pl.modified_model(mg)
    # pinned: the counts of a tick cannot move the ctx to the six-row kernel (sai2b_host.cpp launch_tick)
    env = dict(env) if env else {"SAI2B_NO_SING6": "1"}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        g = pkg.Controller(mg, cg, inp.B, introspection=introspection)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return ol.Oracle(mo, co, inp.B, threads=threads), g


def _inputs(route, B, seed, blend=True):
    return pl.Inputs(ROUTES[route][0], B, seed, blend=blend)


def _run(g, inp, ticks):
    """-> per tick (tau, integrators, bookkeeping [(n, c1, c2) per MFT], fallback count) of a Controller"""
    out = []
    for k in range(ticks):
        pl.feed(g, inp.tasks, inp.at(k))
        tau = g.tick()
        sh = [g.get_mft_singularity_state(t) for t, (kind, _) in enumerate(inp.tasks) if kind == "mft"]
        out.append((tau, pl.integrators(g, inp.tasks), sh, g.fallback_count()))
    return out


class _Oracle:
    """the oracle's side of a run, tick by tick, with what the device should have done"""

    def __init__(self, o, inp):
        self.o, self.inp = o, inp
        self.prev_sing = np.zeros(inp.B, dtype=bool)

    def tick(self, k):
        o, inp = self.o, self.inp
        pl.feed(o, inp.tasks, inp.at(k))
        tau = o.tick()
        sing, grey, sh = np.zeros(inp.B, dtype=bool), np.zeros(inp.B, dtype=bool), []
        for t, (kind, _) in enumerate(inp.tasks):
            if kind != "mft":
                continue
            s, _, ro = o.get_mft_singularity(t)
            rank = o.tasks[t].pos_range + o.tasks[t].ori_range
            _, c1, c2 = o.get_mft_sh_state(t)
            sh.append((rank - ro.astype(int), c1.astype(int), c2.astype(int)))
            sing |= ro < rank
            grey |= (ro == rank) & (s[rank - 1] < GREY * s[0])
        leaving = self.prev_sing & ~sing
        self.prev_sing = sing
        return tau, pl.integrators(o, inp.tasks), sh, sing, leaving, grey


def _check_tick(tag, dev, ora, route):
    tau_g, ig, shg, fb = dev
    tau_o, io, sho, sing, leaving, grey = ora
    e = _err(tau_g, tau_o)
    assert e[~sing].max(initial=0) < TOL, (tag, "torque", np.flatnonzero(e[~sing] >= TOL)[:8], e.max())
    assert e[sing].max(initial=0) < TOL_SINGULAR, (tag, "singular torque", e[sing].max(initial=0))
    for t, (a, b) in enumerate(zip(ig, io)):
        ei = np.abs(a - b).max(axis=0) / np.maximum(np.abs(b).max(axis=0), 1e-300)
        assert ei.max() < TOL_INTEG, (tag, "integrators of task", t, np.flatnonzero(ei >= TOL_INTEG)[:8], ei.max())
    for t, (a, b) in enumerate(zip(shg, sho)):
        for name, x, y in zip(("directions", "type-1 count", "type-2 count"), a, b):
            assert np.array_equal(x, y), (tag, "bookkeeping", t, name, np.flatnonzero(x != y)[:8])
    if route in FAST:
        # the robots that must decline: the singular ones and those leaving a region (istate); a regular robot
        # in the certificate's grey zone may be declined too
        must = int((sing | leaving).sum())
        assert must <= fb <= must + int((grey & ~sing & ~leaving).sum()), (tag, "fallback count", fb, must)


def _parity(route, B, monkeypatch, seed):
    inp = _inputs(route, B, seed)
    o, g = _make(route, inp, monkeypatch, threads=16)
    dev, ora = _run(g, inp, WARMUP + MEASURED), _Oracle(o, inp)
    left = 0
    for k in range(WARMUP + MEASURED):
        res = ora.tick(k)
        _check_tick(f"{route} B={B} tick {k}", dev[k], res, route)
        left += int(res[4].sum())
    # by the end of the warm-up every integrator row the hierarchy advances is non-zero for (nearly) every robot (a
    # JointTask left with no range by the tasks above does not advance its integrators)
    for t, ((kind, _), a) in enumerate(zip(inp.tasks, dev[WARMUP - 1][1])):
        c = o.tasks[t]
        rows = [r for r in range(12) if r < 6 and (c.pos_range, c.ori_range)[r // 3] or r >= 6 and ROUTES[route][1]]
        live = a[rows] if kind == "mft" else a
        assert (live != 0).mean(axis=1).min() >= (0.9 if B >= 64 else 0.0), (route, B, kind)
        assert (live != 0).any(axis=1).all() or B < 64, (route, B, kind)
    assert left >= min(B, 2), "robots must leave the singular region while measured"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_parity_at_ragged_batch_sizes(route, B, monkeypatch):
    _parity(route, B, monkeypatch, seed=900 + B)


@pytest.mark.parametrize("B", BIG)
@pytest.mark.parametrize("route", ["c3", "c4"])
def test_parity_at_large_ragged_batch_sizes(route, B, monkeypatch):
    _parity(route, B, monkeypatch, seed=900 + B)


def _rows_read(inp):
    """every per-robot input row the hierarchy's tick reads: (key, row, ticks it is changed at) with `ticks` = the
    measured tick for the inputs of a tick, the warm-up for the rows that only drive an integrator (the integrator row
    is what is read), None for the istate row (the robot is put into a singular pose at the last warm-up tick)"""
    now, warm = (WARMUP,), tuple(range(WARMUP))
    out = [("q", i, now) for i in range(N)] + [("dq", i, now) for i in range(N)]
    for t, (kind, _) in enumerate(inp.tasks):
        if kind == "mft":
            out += [(f"mft{t}.{key}", r, now) for key, rows in pl.MFT_KEYS for r in range(rows)]
            # integrator rows: position from the position goal, orientation from the rotation goal, force and moment
            # from their goals
            out += [(f"mft{t}.pos", r, warm) for r in range(3)] + [(f"mft{t}.rot", r, warm) for r in (1, 5, 6)]
            out += [(f"mft{t}.f", r, warm) for r in range(3)] + [(f"mft{t}.m", r, warm) for r in range(3)]
            out.append(("istate", t, None))
        else:
            out += [(f"jt{t}.{key}", r, now) for key in ("q", "dq", "ddq") for r in range(N)]
            out += [(f"jt{t}.q", r, warm) for r in range(N)]  # the integrator of joint r
    return out


@pytest.mark.parametrize("B", [4097, 4162])
@pytest.mark.parametrize("route", ["c2", "c3"])
def test_one_robot_per_row(route, B, monkeypatch):
    base = _inputs(route, B, seed=77, blend=False)
    rows = _rows_read(base)
    # one robot per row, the last two robots (the partial wavefront) among them, lanes spread over both halves
    robots = [B - 1, B - 2] + [B - 3 - 45 * j for j in range(len(rows) - 2)]
    assert len(set(robots)) == len(rows) and min(robots) >= 0
    pert = _inputs(route, B, seed=77, blend=False)
    rng = np.random.default_rng(5)
    for (key, row, ticks), r in zip(rows, robots):
        if key == "istate":
            pert.singular[WARMUP - 1] = np.array([r])
        else:
            scale = 1.0 if key.split(".")[-1] in ("f", "m", "sf", "sm") else 0.02
            pert.extra.append((key, row, r, scale * rng.choice([-1, 1]) * rng.uniform(1, 2), ticks))
    robots = np.array(robots)
    mine = np.zeros(B, dtype=bool)
    mine[robots] = True
    ticks = WARMUP + 2
    ob, gb = _make(route, base, monkeypatch, threads=16)
    op, gp = _make(route, pert, monkeypatch, threads=16)
    dev_b, dev_p = _run(gb, base, ticks), _run(gp, pert, ticks)
    ora_b, ora_p = _Oracle(ob, base), _Oracle(op, pert)
    for k in range(ticks):
        rb, rp = ora_b.tick(k), ora_p.tick(k)
        tag = f"{route} B={B} tick {k}"
        (tb, ib, sb, _), (tp, ip, sp, _) = dev_b[k], dev_p[k]
        # the robots nobody touched: bit for bit the baseline
        same = np.all(tb == tp, axis=0)
        for a, b in zip(ib, ip):
            same &= np.all(a == b, axis=0)
        for a, b in zip(sb, sp):
            for x, y in zip(a, b):
                same &= x == y
        assert same[~mine].all(), (tag, "changed without being perturbed", np.flatnonzero(~same & ~mine)[:8])
        # the touched ones: as the oracle has them on the perturbed inputs
        _check_tick(tag, dev_p[k], rp, None)
        if k == WARMUP:
            moved = _err(rp[0], rb[0])[robots]
            assert (moved > 1e-8).all(), (tag, "perturbation not visible", [rows[i] for i in np.flatnonzero(moved <= 1e-8)])
            assert not same[robots].any(), (tag, "perturbed robot unchanged on the device", robots[same[robots]])
        if k == WARMUP and route in FAST:  # the istate robot declined
            assert dev_p[k][3] == dev_b[k][3] + 1, (dev_p[k][3], dev_b[k][3])


@pytest.mark.parametrize("route", list(ROUTES))
def test_results_do_not_depend_on_the_position_in_the_batch(route, monkeypatch):
    """bit for bit on every route: no lane's arithmetic depends on its neighbours, also not in the cert kernel (the
    in-lane singular branch masks the other lanes) and not behind the work list (the 16-lane generic kernel decides
    certified / SVD per robot, where the one-lane tick_kernel<false> would decide per wavefront with __all)"""
    B = 1000  # 15 full wavefronts and one of 40
    inp = _inputs(route, B, seed=31)
    rng = np.random.default_rng(8)
    orders = {"reversed": np.arange(B)[::-1], "rolled": np.roll(np.arange(B), 40), "shuffled": rng.permutation(B),
              "odd subset": np.sort(rng.choice(B, size=577, replace=False))}
    ticks = WARMUP + 3
    _, g = _make(route, inp, monkeypatch)
    ref = _run(g, inp, ticks)
    del g
    for name, idx in orders.items():
        sub = inp.select(idx)
        _, g = _make(route, sub, monkeypatch)
        got = _run(g, sub, ticks)
        del g
        for k in range(ticks):
            (ta, ia, sa, _), (tb, ib, sb, _) = ref[k], got[k]
            tag = f"{route} {name} tick {k}"
            assert np.array_equal(ta[:, idx], tb), (tag, "torques", np.abs(ta[:, idx] - tb).max())
            for a, b in zip(ia, ib):
                assert np.array_equal(a[:, idx], b), (tag, "integrators", np.abs(a[:, idx] - b).max())
            for a, b in zip(sa, sb):
                for x, y in zip(a, b):
                    assert np.array_equal(x[idx], y), (tag, "bookkeeping")


def test_c5_full_size_in_one_ctx_and_in_eight():
    """BASELINE config 5: eight ranks' inputs of 65 536 robots, as one ctx of 524 288 and as eight ctxs on device 0"""
    parts = [pkg.workloads.make_inputs(5, rank=r) for r in range(8)]
    S = parts[0]["B"]
    full = {"tasks": parts[0]["tasks"], "B": 8 * S, "q": np.concatenate([p["q"] for p in parts], axis=1),
            "dq": np.concatenate([p["dq"] for p in parts], axis=1)}
    for key in ("mft0", "jt1"):
        full[key] = {k: np.concatenate([p[key][k] for p in parts], axis=1) for k in parts[0][key]}
    cfg = pkg.task_configs(full["tasks"])
    one = pkg.Controller(pkg.panda_model(), cfg, full["B"], device=0)
    ol.load_inputs(one, full)
    eight = [pkg.Controller(pkg.panda_model(), cfg, S, device=0) for _ in parts]
    for g, p in zip(eight, parts):
        ol.load_inputs(g, p)
    tau1 = [one.tick() for _ in range(3)]
    tau8 = [[g.tick() for g in eight] for _ in range(3)]
    del one, eight
    for k in range(3):
        assert np.array_equal(tau1[k], np.concatenate(tau8[k], axis=1)), k
    for r, p in enumerate(parts):  # the oracle one rank at a time (its per-robot state is large)
        o = ol.Oracle(ol.panda_model(), ol.task_configs(p["tasks"]), S, threads=16)
        ol.load_inputs(o, p)
        for k in range(3):
            e = _err(tau1[k][:, r * S:(r + 1) * S], o.tick())
            assert e.max() < TOL, (r, k, e.max())
        o.close()

"""Every kernel route of a tick for the 4-, 6- and 8-joint robots (-m gpu), on poses spread over the singularity bands of
the hierarchy's MotionForceTask (tests/singular_poses.py) and at ragged batch sizes, against the CPU oracle: torques every
period, the singularity bookkeeping exactly, that the route asked for really ran, joint states at the end.

Routes (each forced by its environment switch before the controller is created):
  default      the SVD-free kernel for general hierarchies with the in-lane singular branch, work list behind it
  no_inlane    the same without the in-lane branch (SAI2B_NO_INLANE_SINGULAR=1): every singular robot takes the work list
  sing6        tick_cert_kernel<6, S6> from the first tick (SAI2B_FORCE_SING6=1; hierarchies with a 6-row task)
  generic16/8  the lanes-per-robot generic kernel over the whole batch, 16 or 8 lanes a robot (SAI2B_NO_CERT_PATH=1)
  introspection  the one-lane kernel
SAI2B_ROBOT_SEEDS=<n> widens the sweep of the closed-loop test over pose seeds (manual runs)."""
import os

import numpy as np
import pytest

import oracle_lib as ol
import singular_poses as sp
import test_gpu_robots as tr

pytestmark = pytest.mark.gpu

HIERARCHIES = {"planar_4r": ("planar_4r", False), "six_r": ("six_r", False), "six_r_mft6": ("six_r", True),
               "sliding_base": ("sliding_base", False)}
ROUTES = {"default": {}, "no_inlane": {"SAI2B_NO_INLANE_SINGULAR": "1"}, "sing6": {"SAI2B_FORCE_SING6": "1"},
          "generic16": {"SAI2B_NO_CERT_PATH": "1", "SAI2B_GENERIC_LANES": "16"},
          "generic8": {"SAI2B_NO_CERT_PATH": "1", "SAI2B_GENERIC_LANES": "8"}, "introspection": {}}
SING6 = ("sliding_base", "six_r_mft6")  # a 6-row task: the hierarchies tick_cert_kernel<6, S6> serves
BATCHES = (1, 63, 65, 4096 + 37)
# a robot whose oracle ratio sits this close (relative) to a threshold may be classified on the other side by the
# kernel's own decomposition: its bookkeeping is exempt, and such robots are counted
ROUNDING_BAND = 1e-7


def _cells():
    for name in HIERARCHIES:
        for route in ROUTES:
            if route == "sing6" and name not in SING6:
                continue
            yield name, route


def _make(name, route, B, q, monkeypatch, seed=0):
    robot, mft6 = HIERARCHIES[name]
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    try:
        return tr._setup(robot, B, False, route == "introspection", seed=seed, q=q, mft6_alone=mft6)
    finally:
        for k in ROUTES[route]:
            monkeypatch.delenv(k)


class _Checker:
    """the per-period assertions against the oracle; keeps the counts the end of a run asserts on"""

    def __init__(self, o, g, kinds, B, route):
        self.o, self.g, self.kinds, self.B, self.route = o, g, kinds, B, route
        self.near = np.zeros(B, dtype=bool)  # ever within ROUNDING_BAND of a threshold: history may differ from then on
        self.near_periods = 0
        self.ever_singular = np.zeros(B, dtype=bool)
        self.periods = 0
        self.in_region = 0
        self.fb = []  # fallback_count() of every period so far

    def period(self, tau_g, tau_o, tag):
        o, g, B = self.o, self.g, self.B
        singular = np.zeros(B, dtype=bool)
        tol_singular = np.full(B, 1e-5)
        n_two = n_sing = 0
        self.max_rank = 0
        for t, k in enumerate(self.kinds):
            if k != "mft":
                continue
            sig, _, ro = o.get_mft_singularity(t)
            rank = o.tasks[t].pos_range + o.tasks[t].ori_range
            self.max_rank = max(self.max_rank, rank)
            ro = ro.astype(int)
            singular |= ro < rank
            n_sing += int((ro < rank).sum())
            n_two += int((ro < rank - 1).sum())
            tol_singular = np.maximum(tol_singular, 1e-16 * (sig[0] / np.maximum(sig[rank - 1], 1e-12)) ** 2)
            rho = sig[:rank] / np.maximum(sig[0], 1e-300)
            near = np.zeros(B, dtype=bool)
            for thr in (sp.S_MIN, sp.S_MAX):
                near |= (np.abs(rho[1:] / thr - 1) < ROUNDING_BAND).any(axis=0)
            near |= np.abs(sig[0] / 1e-3 - 1) < ROUNDING_BAND  # s_abs_tol
            self.near_periods += int(near.sum())
            self.near |= near
            # the bookkeeping: number of singular directions, type-1 and type-2 counts of the history
            n, c1, c2 = g.get_mft_singularity_state(t)
            _, c1o, c2o = o.get_mft_sh_state(t)
            bad = (n != rank - ro) | (c1 != c1o) | (c2 != c2o)
            assert not (bad & ~self.near).any(), (tag, t, np.flatnonzero(bad & ~self.near)[:8], n[bad][:4], (rank - ro)[bad][:4],
                                                  c1[bad][:4], c1o[bad][:4], c2[bad][:4], c2o[bad][:4])
            # (a robot the kernel saw on the other side of a threshold: its torque follows that side)
            singular |= n > 0
        e = tr._err(tau_g, tau_o)
        if (~singular).any():
            assert e[~singular].max() < 1e-9, (tag, e[~singular].max())
        if singular.any():
            assert (e[singular] < tol_singular[singular]).all(), (tag, e[singular].max())
        # the route ran
        fb = g.fallback_count()
        slack = 2 + B // 100
        # the back-off: the host reads the count of the ticks 0, 8, 16, ... eight ticks later; above 40 % of the batch the
        # generic kernel runs alone for the next 64 ticks
        p = self.periods
        backed_off = fb == B and any(self.fb[k] * 5 > 2 * B for k in range(0, p - 7, 8) if k >= p - 72)
        if self.route == "sing6" or (self.route == "default" and self.max_rank <= 3):
            # the in-lane branch keeps every robot with one singular direction (3-row tasks; 6-row ones in tick_cert_kernel<6, S6>)
            assert fb <= n_two + slack or backed_off, (tag, fb, n_two)
        elif self.route == "default":
            # a 4- to 6-row task outside the S6 kernel: the singular robots take the work list
            assert fb <= n_sing + slack or backed_off, (tag, fb, n_sing)
        elif self.route == "no_inlane":
            assert fb >= min(n_sing, 1) and (fb >= n_sing or fb == B), (tag, fb, n_sing)
        elif self.route.startswith("generic"):
            assert fb == B, (tag, fb)
        self.fb.append(fb)
        self.ever_singular |= singular
        self.in_region += int(singular.sum())
        self.periods += 1

    def finish(self):
        o, g, B = self.o, self.g, self.B
        qo, vo = o.get_state()
        qg, vg = g.get_state()
        ok = ~self.ever_singular
        if ok.any():
            assert np.abs(qo - qg)[:, ok].max() < 1e-10 and np.abs(vo - vg)[:, ok].max() < 1e-8
        assert self.near.sum() <= 1 + B * self.periods // 1000, (self.near.sum(), self.near_periods)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name,route", list(_cells()))
@pytest.mark.parametrize("seed", range(int(os.environ.get("SAI2B_ROBOT_SEEDS", "1"))))
def test_route_matches_the_oracle_in_closed_loop(name, route, B, seed, monkeypatch):
    """20 control periods through the simulation harness from poses of every band of the hierarchy's task"""
    q, band = sp.mixed(name, B, seed=seed)
    m, kinds, o, g, _, _ = _make(name, route, B, q, monkeypatch, seed=seed)
    chk = _Checker(o, g, kinds, B, route)
    for period in range(20):
        tau_o, tau_g = o.tick(), g.tick()
        chk.period(tau_g, tau_o, period)
        for c in (o, g):
            c.sim_step(tau_o, 0.001, 1, with_gravity=False)
    chk.finish()
    if len(sp.TASKS[name]["bands"]) > 1 and B > 1:
        assert chk.in_region > 0


@pytest.mark.parametrize("name,route", [c for c in _cells() if c[1] != "introspection"])
def test_route_follows_robots_into_the_region_and_out_again(name, route, monkeypatch):
    """robots carried from a regular pose into the blending region (some through it to the singular pose) and back over
    32 ticks: entering, the history ring, the type-1 / type-2 switch and the clearing on the way out, tick by tick"""
    B = 65
    bands = sp.TASKS[name]["bands"]
    deep = "two" if "two" in bands else "inside"
    q_s = sp.poses(name, deep, 16)[:, np.arange(B) % 16]
    q_r = sp.poses(name, "regular", 16)[:, np.arange(B) % 16]
    m, kinds, o, g, _, dq = _make(name, route, B, q_r, monkeypatch)
    reach = np.linspace(0.8, 1.0, B)  # how far towards the pose of the deep band each robot goes
    chk = _Checker(o, g, kinds, B, route)
    seen_in = seen_out = 0
    for tick in range(32):
        s = reach * (1 - np.cos(2 * np.pi * tick / 32)) / 2
        q = np.ascontiguousarray(q_r + s * (q_s - q_r))
        for c in (o, g):
            c.set_state(q, 0.2 * dq)
        tau_o, tau_g = o.tick(), g.tick()
        _, _, ro = o.get_mft_singularity(kinds.index("mft"))
        rank = o.tasks[kinds.index("mft")].pos_range + o.tasks[kinds.index("mft")].ori_range
        seen_in += int((ro < rank).sum())
        seen_out += int((ro == rank).sum())
        chk.period(tau_g, tau_o, tick)
    assert seen_in > B and seen_out > 4 * B, (seen_in, seen_out)
    assert chk.near.sum() <= 1 + B * chk.periods // 1000


def test_back_off_selects_the_eight_lane_generic_kernel_on_a_big_unfiltered_batch():
    """the sliding-base hierarchy on 16 384 unfiltered poses, nothing forced: the SVD-free kernel declines most of the batch,
    the host reads that count at tick 8 (the probe of tick 0) and runs the generic kernel over the whole batch — with 8
    lanes a robot, the choice for B >= 16 384 — from then on; torques as the oracle's throughout"""
    B = 16384
    m, kinds, o, g, q, dq = tr._setup("sliding_base", B, False, False, seed=11)
    chk = _Checker(o, g, kinds, B, "back_off")
    seen = []
    for tick in range(12):
        tau_o, tau_g = o.tick(), g.tick()
        chk.period(tau_g, tau_o, tick)
        seen.append(g.fallback_count())
        for c in (o, g):
            c.sim_step(tau_o, 0.001, 1, with_gravity=False)
    assert B * 0.4 < seen[0] < B, seen  # the SVD-free kernel ran first and declined most robots ...
    assert all(s == B for s in seen[8:]), seen  # ... and the probe of tick 0, read at tick 8, sent the batch to the generic kernel
    chk.finish()


def _takeover_run(inp, ramp):
    import test_gpu_cert_kernel as tc

    B = inp["B"]
    _, g = tc._pair(inp)
    ol.load_inputs(g, inp)
    taus, states, fbs = [], [], []
    for tick, k in enumerate(ramp):
        q = inp["q"].copy()
        q[3, :k] = -0.0698 - 0.002 * (np.arange(k) % 7)  # elbow at its limit: inside the 6-row task's blending region
        g.set_state(q, inp["dq"])
        if tick % 8 == 7:
            taus.append(g.tick())
            states.append(g.get_mft_singularity_state(0))
            fbs.append(g.fallback_count())
        else:
            g.tick(want_output=False)
    g.synchronize()
    return taus, states, fbs


def test_route_switching_is_a_function_of_the_tick_index():
    """[MFT(6), JT(7)] on 49 152 Panda robots (the benchmark's regular poses) of which a growing share is moved into a blending
    region and back out, over 80 ticks: the batch crosses the takeover of tick_cert_kernel<6, S6> (20 480 declined) and the
    way back (15 360) within the run. Two runs in fresh controllers, torques fetched only every 8th tick, must agree bit
    for bit: the route of tick k is decided by the counts of tick k - 8 alone, whenever their read-back arrives"""
    import sai2_primitives_perso_amd as pkg

    B = 49152
    inp = pkg.workloads.make_inputs(3, B=B, seed=903)
    frac = np.concatenate([np.linspace(0, 0.8, 24), np.full(16, 0.8), np.linspace(0.8, 0.15, 16), np.full(24, 0.15)])
    ramp = (frac * B).astype(int)
    a = _takeover_run(inp, ramp)
    b = _takeover_run(inp, ramp)
    for ta, tb in zip(a[0], b[0]):
        assert np.array_equal(ta, tb)
    for sa, sb in zip(a[1], b[1]):
        assert all(np.array_equal(x, y) for x, y in zip(sa, sb))
    assert a[2] == b[2]
    fbs, inside = a[2], ramp[7::8]
    # probes at ticks 0, 8, 16, ... act at 8, 16, 24, ...: the probe of tick 16 (27 000 declined) switches at tick 24, the one
    # of tick 56 (7 400 in the region) back at tick 64. Fetched ticks 7, 15, 23: the headline kernel declines every robot in
    # the region; 31 ... 63: the 6-row kernel keeps them; 71, 79: the headline kernel again
    for k in range(3):
        assert fbs[k] >= inside[k], (fbs, inside)
    for k in range(3, 8):
        assert fbs[k] < 0.1 * inside[k], (fbs, inside)
    for k in range(8, 10):
        assert fbs[k] >= inside[k], (fbs, inside)

"""-m gpu: the device trajectory planners against the reference's ruckig, input row by input row, for generators of
1 .. 7 DoFs (7-joint build) and 1 .. 8 DoFs (8-joint build: SAI2B_OTG_MAXD = 8, every lane of a group active).

The planners run in a test-only harness (tests/cpp/otg_planner_device.hip) built like sai2b_otg_n*.o: the group forms
otgg::calculate / calculate3 (one DoF per lane, the synchronisation by shuffles and ballots; what otg_plan_kernel and
otg3_plan_kernel<false> run), the sequential forms on one device lane (what plan_lane3 runs) and the sequential forms on
the host. The rows (tests/otg_planner_rows.py) reach the branches where ruckig's synchronisation separates: brake
pre-trajectories, non-zero and +-vmax target velocities, blocked intervals deciding the duration, collinear and just
off collinear inputs, exact ties, durations on either side of the 7.6e3 s limit, tiny displacements, jerk 1e-1 .. 1e6.

Tolerances. The acceleration-limited planner is +, -, *, / and sqrt without contraction: device and ruckig agree bit
for bit. The jerk-limited planner's root finders call cbrt / acos / cos, which on the device come from another math
library than glibc's; their last bits differ, so device vs ruckig is held to 1e-9 (durations relative to max(1, T),
samples relative to max(1, |ref|)) with the same profile kinds (limits / direction / control signs) as the host build.
Group vs one-lane on the device share that library and must agree bit for bit.
"""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest

import oracle_lib as ol
import otg_planner_rows as op  # (puts tests/golden on the path)
import otg_np  # noqa: E402

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not os.path.exists(op.HIPCC) and shutil.which("hipcc") is None, reason="hipcc not found"),
    pytest.mark.skipif(not otg_np.ref_available(), reason="oracle/_ref/libruckig_ref.so not built"),
]

BUILDS = (7, 8)
REPORT = {}


@pytest.fixture(scope="module")
def ref():
    return otg_np.load_ref()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("otg_planner")
    return {N: op.build_harness(N, str(d / f"libotg_planner_n{N}.so")) for N in BUILDS}


_cache = {}


@pytest.fixture(scope="module")
def rows(harness, ref):
    """per build: the rows, ruckig's answers and every harness path's answers on the compact batch"""
    if not _cache:
        for N in BUILDS:
            n, X, frac, fam = op.families(N, ref)
            d = {"n": n, "X": X, "frac": frac, "fam": fam}
            for jerk in (False, True):
                d["ref", jerk] = op.reference(ref, jerk, n, X, frac)
            for path in op.PATHS:
                d[path] = op.run(harness[N], path, n, X, frac)
            _cache[N] = d
    return _cache


def _report(key, value):
    REPORT[key] = value
    out = os.environ.get("OTG_PLANNER_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def _active(n):
    return np.arange(op.W)[None, :] < n[:, None]


def _first_bad(mask, d):
    i = int(np.nonzero(mask)[0][0])
    return dict(row=i, fam=str(d["fam"][i]), n=int(d["n"][i]), inputs=d["X"][i][:, : d["n"][i]].tolist())


@pytest.mark.parametrize("N", BUILDS)
@pytest.mark.parametrize("jerk", [False, True], ids=["acc", "jerk"])
def test_host_build_is_bit_equal_to_ruckig(rows, N, jerk):
    """the anchor: the sequential planner compiled for the host in the same library equals ruckig bit for bit.

    One allowance, jerk-limited only: this library's host half is compiled by hipcc's clang, ruckig by g++, and the two
    compilers build ruckig's own closed forms of PositionThirdOrderStep2 to different last bits on rare rows (ruckig
    compiled with clang reproduces the clang answer exactly; on the g++ build of the same planner, tests/test_otg3_core.py
    is bit-equal). Those rows keep the result code and duration and may differ in their samples by 1e-12 relative."""
    d = rows[N]
    h, r = d["host_jerk" if jerk else "host_acc"], d["ref", jerk]
    assert (r["res"] != -100).all(), "every row is a valid input"
    assert np.array_equal(h["res"], r["res"]) and np.array_equal(h["dur"], r["dur"])
    bad = np.any(h["pva"] != r["pva"], axis=(1, 2, 3))
    if jerk:
        e = np.abs(h["pva"] - r["pva"]) / np.maximum(1.0, np.abs(r["pva"]))
        _report(f"host_jerk_n{N}", {"rows_not_bit_equal": int(bad.sum()), "max_rel_sample": float(e.max())})
        assert bad.sum() <= 2 and e.max() <= 1e-12, (int(bad.sum()), float(e.max()))
    else:
        assert not bad.any(), (int(bad.sum()), _first_bad(bad, d))


@pytest.mark.parametrize("N", BUILDS)
def test_families_reach_their_branches(rows, N):
    """each family reaches what it targets, in numbers; every family is drawn at every n it applies to"""
    d = rows[N]
    n, fam = d["n"], d["fam"]
    for f in np.unique(fam):
        want = {1} if f == "blocked_single" else set(range(2 if f in ("collinear", "near_collinear", "ties", "blocked") else 1, N + 1))
        assert want <= set(n[fam == f].tolist()), f
    for jerk in (False, True):
        host, r = d["host_jerk" if jerk else "host_acc"], d["ref", jerk]
        cov = op.coverage(n, fam, host, op.blocked_rows(n, fam, r["dur"], r["res"]))
        _report(f"coverage_n{N}_{'jerk' if jerk else 'acc'}", cov)
        assert cov["brake"] >= 300 and cov["phase_synced"] >= 500 and cov["blocked"] >= 25 and cov["err_duration"] >= 15, cov


@pytest.mark.parametrize("N", BUILDS)
@pytest.mark.parametrize("path", ["group_acc", "lane_acc"])
def test_acceleration_limited_device_planner_is_bit_equal_to_ruckig(rows, N, path):
    d = rows[N]
    g, r, h = d[path], d["ref", False], d["host_acc"]
    bad = (g["res"] != r["res"]) | (g["dur"] != r["dur"]) | np.any(g["pva"] != r["pva"], axis=(1, 2, 3))
    assert not bad.any(), (int(bad.sum()), _first_bad(bad, d))
    for k in ("meta", "bdur", "tph"):
        assert np.array_equal(g[k], h[k]), k


@pytest.mark.parametrize("N", BUILDS)
def test_jerk_limited_group_planner_is_bit_equal_to_the_one_lane_planner(rows, N):
    """same math library on both sides: any difference is in the synchronisation over the lanes"""
    d = rows[N]
    g, lane = d["group_jerk"], d["lane_jerk"]
    for k in ("res", "dur", "meta", "bdur", "tph", "pva"):
        bad = np.any((g[k] != lane[k]).reshape(len(d["n"]), -1), axis=1)
        assert not bad.any(), (k, int(bad.sum()), _first_bad(bad, d))


@pytest.mark.parametrize("N", BUILDS)
@pytest.mark.parametrize("path", ["group_jerk", "lane_jerk"])
def test_jerk_limited_device_planner_follows_ruckig(rows, N, path):
    d = rows[N]
    g, r, h = d[path], d["ref", True], d["host_jerk"]
    assert np.array_equal(g["res"], r["res"]), _first_bad(g["res"] != r["res"], d)
    dT = np.abs(g["dur"] - r["dur"]) / np.maximum(1.0, r["dur"])
    ds = np.abs(g["pva"] - r["pva"]) / np.maximum(1.0, np.abs(r["pva"]))
    act = _active(d["n"])
    for k in ("meta",):
        bad = np.any((g[k] != h[k]) & act[:, None, :], axis=(1, 2))
        assert not bad.any(), (k, int(bad.sum()), _first_bad(bad, d))
    _report(f"jerk_{path}_n{N}", {"max_rel_dT": float(dT.max()), "max_rel_sample": float(ds.max()),
                                  "rows_not_bit_equal": int(np.sum((g["dur"] != r["dur"]) | np.any(g["pva"] != r["pva"], axis=(1, 2, 3))))})
    assert dT.max() <= 1e-9 and ds.max() <= 1e-9, (dT.max(), ds.max())


@pytest.mark.parametrize("N", BUILDS)
@pytest.mark.parametrize("path", ["group_acc", "group_jerk", "lane_acc", "lane_jerk"])
def test_every_row_gives_the_same_answer_wherever_it_sits(rows, harness, N, path):
    """(b) shuffled into 65 536 rows with neighbours of other n in the same wavefront, (c) a batch of 8k + 5 rows,
    (d) inactive lanes padded with NaN and +-1e300: bit-identical to the compact run"""
    d = rows[N]
    n, X, frac = d["n"], d["X"], d["frac"]
    R = len(n)
    base = d[path]
    rng = np.random.default_rng(N * 10 + list(op.PATHS).index(path))

    def check(idx, got, what):
        for k in ("res", "dur", "meta", "bdur", "tph", "pva"):
            bad = np.any((got[k] != base[k][idx]).reshape(len(idx), -1), axis=1)
            assert not bad.any(), (what, k, int(bad.sum()), _first_bad(np.isin(np.arange(R), idx[bad]), d))

    idx = rng.permutation(np.concatenate([np.arange(R), rng.integers(0, R, 65536 - R)]))
    check(idx, op.run(harness[N], path, n[idx], X[idx], frac[idx]), "65536 shuffled")
    idx = rng.permutation(R)[: (R // 2) // 8 * 8 + 5]
    check(idx, op.run(harness[N], path, n[idx], X[idx], frac[idx]), "8k+5")
    Xp = X.copy()
    pad = ~_active(n)
    fill = rng.choice(np.array([np.nan, 1e300, -1e300]), size=Xp.shape)
    Xp[np.broadcast_to(pad[:, None, :], Xp.shape)] = fill[np.broadcast_to(pad[:, None, :], Xp.shape)]
    check(np.arange(R), op.run(harness[N], path, n, Xp, frac), "NaN / 1e300 padding")


# ---- the wrapper stepped tick by tick against the oracle's OTG_joints ----
K_TICKS = 1200


def _stepped_trials(N, T, seed):
    """per trial: n, x0, limits (vmax, amax, jmax), per-tick goals and set flags. Goals with target velocities (the
    Finished-with-velocity re-goal), new goals while moving, a goal repeated exactly and one within 1e-13 (no-ops)"""
    rng = np.random.default_rng(seed)
    W = op.W
    n = np.array([1 + t % N for t in range(T)], np.int32)
    x0, lim = np.zeros((T, W)), np.zeros((T, 3, W))
    gp, gv, flag = np.zeros((T, K_TICKS, W)), np.zeros((T, K_TICKS, W)), np.zeros((T, K_TICKS), np.int32)
    for t in range(T):
        k = n[t]
        x0[t, :k] = rng.normal(0, 1, k)
        vm, am, jm = rng.uniform(1, 4, k), rng.uniform(5, 30, k), rng.uniform(100, 2000, k)
        lim[t, 0, :k], lim[t, 1, :k], lim[t, 2, :k] = vm, am, jm
        every_tick = t % 2 == 0  # the product sets the task's goal every tick
        g = x0[t, :k] + rng.normal(0, 0.3, k)
        v = rng.uniform(-0.6, 0.6, k) * vm if t % 3 else np.zeros(k)
        changes = {0: (g, v), int(rng.integers(150, 400)): (g + rng.normal(0, 0.2, k), np.zeros(k))}
        t2 = int(rng.integers(450, 600))
        g2, v2 = g + rng.normal(0, 0.3, k), rng.uniform(-0.5, 0.5, k) * vm * (t % 4 != 1)
        changes[t2] = (g2, v2)
        changes[t2 + 120] = (g2.copy(), v2.copy())  # repeated exactly
        changes[t2 + 240] = (g2 * (1 + 1e-13), v2 * (1 + 1e-13))  # within isApprox's 1e-12: no new goal
        changes[int(rng.integers(820, 900))] = (g2 + rng.normal(0, 0.2, k), np.zeros(k))
        cur = None
        for tick in range(K_TICKS):
            if tick in changes:
                cur = changes[tick]
                flag[t, tick] = 1
            elif every_tick:
                flag[t, tick] = 1
            gp[t, tick, :k], gv[t, tick, :k] = cur
    return n, x0, lim, gp, gv, flag


def _oracle_stepped(N, jerk, n, x0, lim, gp, gv, flag):
    L = ol.lib(N)
    L.otg_test_joints_create.restype = C.c_void_p
    L.otg_test_joints_create.argtypes = [C.c_int, C.c_void_p, C.c_double]
    for f in ("otg_joints_set_goal", "otg_joints_set_limits"):
        getattr(L, f).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.otg_joints_set_max_jerk.argtypes = [C.c_void_p, C.c_void_p]
    L.otg_joints_update.argtypes = [C.c_void_p]
    L.otg_test_joints_get.argtypes = [C.c_void_p] * 6
    T = len(n)
    pva, rg = np.zeros((T, K_TICKS, 3, op.W)), np.zeros((T, K_TICKS, 2), np.int32)
    gpc, gvc = np.ascontiguousarray(gp), np.ascontiguousarray(gv)
    buf = np.zeros((3, op.W))
    ints = np.zeros(2, np.int32)
    pb, vb, ab = (buf[q].ctypes.data for q in range(3))
    for t in range(T):
        k = int(n[t])
        x = np.ascontiguousarray(x0[t, :k])
        lt = np.ascontiguousarray(lim[t])
        h = L.otg_test_joints_create(k, x.ctypes.data, 0.001)
        L.otg_joints_set_limits(h, lt[0].ctypes.data, lt[1].ctypes.data)
        if jerk:
            L.otg_joints_set_max_jerk(h, lt[2].ctypes.data)
        for tick in range(K_TICKS):
            if flag[t, tick]:
                L.otg_joints_set_goal(h, gpc[t, tick].ctypes.data, gvc[t, tick].ctypes.data)
            L.otg_joints_update(h)
            L.otg_test_joints_get(h, pb, vb, ab, ints.ctypes.data + 4, ints.ctypes.data)  # (goal_reached, result)
            pva[t, tick, :, :k] = buf[:, :k]
            rg[t, tick] = ints
        C.CDLL(None).free(C.c_void_p(h))
    return pva, rg


@pytest.mark.parametrize("N,trials", [(7, 128), (8, 256)])
@pytest.mark.parametrize("jerk", [False, True], ids=["acc", "jerk"])
def test_stepped_wrapper_follows_the_oracle(harness, N, trials, jerk):
    """otgg::joints_set_goal + otgg::update (LaneGen / LaneGen3), 1 200 ticks per trial, against the oracle's OTG_joints
    (bit-pinned to ruckig; for the jerk-limited generator its planner is ruckig itself)"""
    if jerk and not ol.lib(N).otg_jerk_planner_available():
        pytest.skip("oracle/_ref/libruckig_ref.so not built")
    n, x0, lim, gp, gv, flag = _stepped_trials(N, trials, seed=N * 2 + jerk)
    T = len(n)
    pva, rg = np.zeros((T, K_TICKS, 3, op.W)), np.zeros((T, K_TICKS, 2), np.int32)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    P = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))
    err = harness[N].otgh_stepped(int(jerk), T, K_TICKS, 0.001, P(n, C.c_int), P(x0, C.c_double), P(lim, C.c_double), P(gp, C.c_double),
                                  P(gv, C.c_double), P(flag, C.c_int), pva.ctypes.data_as(dp), rg.ctypes.data_as(ip))
    assert err == 0
    opva, org = _oracle_stepped(N, jerk, n, x0, lim, gp, gv, flag)
    bad = np.any(rg != org, axis=(1, 2))
    assert not bad.any(), ("result / goal_reached", np.nonzero(bad)[0][:5], np.argwhere(rg != org)[:5].tolist())
    reached = rg[:, -1, 1].sum()
    regoal = int(((rg[:, :, 0] == 1) & (rg[:, :, 1] == 0)).sum())  # Finished with velocity: re-goaled to a stop
    if jerk:
        e = np.abs(pva - opva) / np.maximum(1.0, np.abs(opva))
        _report(f"stepped_jerk_n{N}", {"max_rel": float(e.max()), "trials_at_goal": int(reached)})
        assert e.max() <= 1e-9, e.max()
    else:
        bad = np.any(pva != opva, axis=(1, 2, 3))
        assert not bad.any(), (np.nonzero(bad)[0][:5], float(np.abs(pva - opva).max()))
    assert reached >= T // 4 and regoal > 0, (reached, regoal)

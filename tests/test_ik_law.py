"""The inverse-kinematics law's own header (csrc/sai2b_ik_law.h) on the CPU against tests/ik_reference.py, no GPU:
tests/cpp/ik_driver.cpp includes the header alone and is built with plain g++, and once more with -fsanitize=address,undefined
-fno-sanitize-recover=all; each build is run as the stand-alone program it is.

1: one iteration, 10 000 random records per robot size (20 configurations of 500: random axes masks, rot_length, mu0, step_max,
   rest weight, limits on and off with a margin; goals at reachable poses, seeds in and beyond the limits, some at the goal's own q,
   some robots with a NaN or an infinity in the goal, the seed or the rest posture): q_out and status within 1e-12 of the reference on
   the separated records, flags exact; a non-finite robot's outputs untouched.
2: restart seeds, a driver mode of their own: bit-equal to the reference.
3: full solves from near seeds, 2 000 records per size, 40 iterations, tolerances 1e-6: the reference converges on every record
   (tests/test_ik_reference.py), the header converges on every record, the reference's own FK at the header's q_out meets the
   tolerances, flags equal. AGREEMENT in q_out over many iterations, on the separated records whose weighted Jacobian keeps its
   smallest singular value >= 0.05 along the reference's path: MEASURED (g++ -O1, x86-64, against numpy): worst 1.72e-12 (planar 4R
   6.0e-14, 6R 2.9e-15, Panda 4.9e-15, sliding base 1.72e-12; over all separated robots whatever their conditioning 1.8e-11);
   asserted at ten times the worst, 1.72e-11 (ik_cases.Q_BOUND), since g++ and hipcc contract FMAs differently. Far below the cap
   of 1e-9, so the conditioning bound stays at 0.05.
4: far seeds with 8 restarts, 500 Pandas: flags and the index of the winning start equal the reference's on the separated
   records; every robot flagged converged meets the tolerances by the reference's FK."""
import os
import subprocess

import numpy as np
import pytest

import ik_cases as ic
from ik_reference import CONVERGED, NONFINITE, SEPARATION

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sai2-primitives-perso_amd", "csrc")
DRIVER = os.path.join(HERE, "cpp", "ik_driver.cpp")
SAN = "-fsanitize=address,undefined"
TOL = 1e-12
CONFIGS, PER_CONFIG = 20, 500
SENTINEL = -7.25

_built = {}


def _build(tmp_factory, sanitize):
    if sanitize not in _built:
        exe = os.path.join(str(tmp_factory.mktemp("ik" + ("s" if sanitize else ""))), "ik_driver")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe]
        if sanitize:
            cmd[3:3] = [SAN, "-fno-sanitize-recover=all"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _built[sanitize] = exe
    return _built[sanitize]


def _run(exe, tmp_path, mode, ints, vals):
    a, b, c = (str(tmp_path / n) for n in ("ints.bin", "vals.bin", "out.bin"))
    np.ascontiguousarray(ints, dtype=np.int32).tofile(a)
    np.ascontiguousarray(vals, dtype=np.float64).tofile(b)
    r = subprocess.run([exe, mode, a, b, c], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(c, dtype=np.float64).reshape(len(ints), ic.OUT)


# ---------------------------------------------------------------------------------------------- 1: one iteration
_one = []


def _one_iteration_records():
    """[(robot, ints, values, [(reference result, n, nonfinite robots)] per configuration)], drawn and solved once for both builds"""
    if not _one:
        rng = np.random.default_rng(20261021)
        for robot in ic.ROBOTS:
            lo, hi = ic.limits(robot)
            n = len(lo)
            ints, vals, refs = [], [], []
            for g in range(CONFIGS):
                axes = ic.axes_of(robot) if g == 0 else int(rng.integers(1, 64))
                cfg = dict(axes=axes, rot_length=float(rng.uniform(0.1, 1.0)), max_iterations=1, mu0=float(10 ** rng.uniform(-3, -1)),
                           step_max=float(rng.uniform(0.05, 0.6)), use_limits=bool(g % 2 == 0), limit_margin=float(rng.uniform(0, 0.05)) if g % 4 == 0 else 0.0,
                           rest_weight=float(rng.uniform(0.01, 0.5)) if g % 3 == 1 else 0.0)
                ref = ic.reference(robot, **cfg)
                K = PER_CONFIG
                qt = lo[:, None] + (hi - lo)[:, None] * rng.random((n, K))
                goal = ic.reference(robot).goal_rows(qt)
                goal[:3] += rng.normal(size=(3, K)) * 0.05
                seed = lo[:, None] + (hi - lo)[:, None] * rng.uniform(-0.05, 1.05, (n, K))
                seed[:, ::25] = qt[:, ::25]  # at the goal's own q
                goal[:, ::25] = ic.reference(robot).goal_rows(qt)[:, ::25]
                rest = lo[:, None] + (hi - lo)[:, None] * rng.random((n, K)) if cfg["rest_weight"] > 0 else None
                bad = np.nonzero(rng.random(K) < 0.03)[0]
                for b in bad:
                    target = (goal, seed) if rest is None else (goal, seed, rest)
                    t = target[int(rng.integers(len(target)))]
                    t[int(rng.integers(t.shape[0])), b] = rng.choice([np.nan, np.inf, -np.inf])
                out = ref.solve(goal if rest is None else np.concatenate([goal, rest]), seed)
                i, v = ic.pack(robot, ref, goal, seed, rest)
                ints.append(i), vals.append(v), refs.append((out, n, bad))
            _one.append((robot, np.concatenate(ints), np.concatenate(vals), refs))
    return _one


@pytest.mark.parametrize("sanitize", [False, True])
def test_one_iteration_equals_the_restatement(tmp_path_factory, tmp_path, sanitize):
    exe = _build(tmp_path_factory, sanitize)
    worst, seen, dropped, total = 0.0, set(), 0, 0
    for robot, ints, vals, refs in _one_iteration_records():
        got = _run(exe, tmp_path, "law", ints, vals)
        assert len(got) == CONFIGS * PER_CONFIG == 10000
        for g, (out, n, bad) in enumerate(refs):
            o = got[g * PER_CONFIG : (g + 1) * PER_CONFIG]
            what = (robot, g)
            flags = o[:, 13].astype(np.uint8)
            sep = out["sep"] >= SEPARATION
            nf = out["flags"] == NONFINITE
            assert set(np.nonzero(nf)[0]) == set(bad), what
            assert np.array_equal(flags[nf], out["flags"][nf]) and (o[nf, :n] == SENTINEL).all() and (o[nf, 8:13] == SENTINEL).all(), what
            ok = sep & ~nf
            dropped, total = dropped + int((~sep & ~nf).sum()), total + int((~nf).sum())
            assert np.array_equal(flags[ok], out["flags"][ok]), what
            seen |= set(flags.tolist())
            err = max(np.abs(o[ok, :n].T - out["q"][:, ok]).max(), np.abs(o[ok, 8:13].T - out["status"][:, ok]).max())
            worst = max(worst, err)
            assert err < TOL, (what, err)
            assert set(out["status"][2, ok].tolist()) <= {0.0, 1.0} and (out["status"][3, ok] == 0).all()
    print(f"worst {worst:.2e}; flag bytes seen {sorted(seen)}; without separation {dropped} of {total}")
    assert dropped <= ic.MAX_DROPPED * total
    assert {1, 2, 8} <= seen and any(f & 4 for f in seen)


# ---------------------------------------------------------------------------------------------- 2: restart seeds
@pytest.mark.parametrize("sanitize", [False, True])
def test_restart_seeds_are_bit_equal(tmp_path_factory, tmp_path, sanitize):
    exe = _build(tmp_path_factory, sanitize)
    for robot in ic.ROBOTS:
        n = len(ic.limits(robot)[0])
        for start in (1, 5, 16):
            ref = ic.reference(robot, restarts=start, seed=0xFEDCBA9876543210, first_robot=4_000_000_000, draw_id=77, limit_margin=0.03)
            robots = np.arange(300, 700)
            zeros = np.zeros((n, len(robots)))
            ints, vals = ic.pack(robot, ref, np.zeros((12, len(robots))), zeros, robots=robots)
            got = _run(exe, tmp_path, "seeds", ints, vals)
            assert np.array_equal(got[:, :n], ref.restart_seed(start, robots)), (robot, start)


# ---------------------------------------------------------------------------------------------- 3: full solves, near seeds
@pytest.mark.parametrize("sanitize", [False, True])
@pytest.mark.parametrize("robot", ic.ROBOTS)
def test_full_solves_from_near_seeds(tmp_path_factory, tmp_path, robot, sanitize):
    exe = _build(tmp_path_factory, sanitize)
    B = 2000
    case, out = ic.solved(robot, "near", B, **ic.NEAR)
    ref = ic.reference(robot, **ic.NEAR)
    n = ref.dof
    assert (out["flags"] & CONVERGED).all()  # the condition on the inputs
    got = _run(exe, tmp_path, "law", *ic.pack(robot, ref, case["goal"], case["seed"]))
    flags = got[:, 13].astype(np.uint8)
    assert (flags & CONVERGED).all()
    ep, er = ref.pose_error(case["goal"], got[:, :n].T)
    assert (ep <= 1e-6).all() and (er <= 1e-6).all()
    sep = ic.separated(out)
    assert np.array_equal(flags[sep], out["flags"][sep])
    cond = sep & (out["sigma_min"] >= ic.SIGMA_MIN)
    assert np.array_equal(got[cond, 10], out["status"][2, cond])  # the iteration counts
    worst = np.abs(got[cond, :n].T - out["q"][:, cond]).max()
    print(f"{robot}: worst |q_header - q_reference| {worst:.2e} over {cond.sum()} robots with sigma_min >= {ic.SIGMA_MIN}; "
          f"over all separated robots {np.abs(got[sep, :n].T - out['q'][:, sep]).max():.2e}")
    assert cond.sum() >= B // 4
    assert worst <= ic.Q_BOUND


# ---------------------------------------------------------------------------------------------- 4: far seeds, restarts
def test_far_seeds_with_restarts_pick_the_same_start(tmp_path_factory, tmp_path):
    exe = _build(tmp_path_factory, False)
    B = 500
    case, out = ic.solved("panda", "far", B, **ic.FAR)
    ref = ic.reference("panda", **ic.FAR)
    got = _run(exe, tmp_path, "law", *ic.pack("panda", ref, case["goal"], case["seed"]))
    sep = ic.separated(out)
    assert np.array_equal(got[sep, 13].astype(np.uint8), out["flags"][sep])
    # (not the iteration counts: a start that crosses a singular region at mu_min amplifies a rounding to 1e-9 in E, and a later
    # decision may then fall the other way; the two paths join again, a few iterations apart)
    assert np.array_equal(got[sep, 11], out["status"][3, sep])
    assert (out["status"][3] > 0).any()
    ep, er = ref.pose_error(case["goal"], got[:, :7].T)
    cv = (got[:, 13].astype(np.uint8) & CONVERGED) != 0
    assert (ep[cv] <= 1e-6).all() and (er[cv] <= 1e-6).all()

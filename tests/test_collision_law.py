"""The collision-proximity law (csrc/sai2b_collision_law.h, the code collision_kernel runs per lane) against its numpy restatement
(tests/collision_reference.py) on the CPU. tests/cpp/collision_driver.cpp includes the header alone and is built with plain g++,
and once more with -fsanitize=address,undefined, each run as the stand-alone program it is.

10 000 random records per robot size (planar_4r 4, six_r 6, Panda 7, sliding_base 8 joints; seed 20261021), in 100 geometries of
100 robots each: 1 to 16 spheres on random links (-1 included), 0 to 2 planes, 0 to 4 obstacles, random masks and margins, a
pitched base for a third of the geometries, a NaN somewhere in plane 0 or obstacle 0 for a tenth of the robots, a q that is not
finite for one robot in fifty. Distances, normals, gradients and centres within 1e-12 (the bound the project holds pose rows to),
indices and flags exact (a robot whose q is not finite: the flags alone). The records are held to the separation the GPU cells are held to (runner-up 1e-9 above the winner,
margins 1e-9 away, normalised distances above 1e-3 m): with continuous draws a violation is a matter of chance, and the remedy
is another seed."""
import os
import subprocess

import numpy as np
import pytest

import collision_cases as cc
import sai2_primitives_perso_amd as pkg
from collision_reference import CollisionReference, product_spheres

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "sai2-primitives-perso_amd", "csrc")
DRIVER = os.path.join(HERE, "cpp", "collision_driver.cpp")
SAN = "-fsanitize=address,undefined"
INTS, IN, OUT = 45, 199, 88
TOL = 1e-12
GEOMETRIES, PER_GEOMETRY = 100, 100

_built = {}


def _build(tmp_factory, sanitize):
    if sanitize not in _built:
        exe = os.path.join(str(tmp_factory.mktemp("col" + ("s" if sanitize else ""))), "collision_driver")
        cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe]
        if sanitize:
            cmd[3:3] = [SAN, "-fno-sanitize-recover=all"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        _built[sanitize] = exe
    return _built[sanitize]


def _run(exe, tmp_path, ints, vals):
    a, b, c = (str(tmp_path / n) for n in ("ints.bin", "vals.bin", "out.bin"))
    np.ascontiguousarray(ints, dtype=np.int32).tofile(a)
    np.ascontiguousarray(vals, dtype=np.float64).tofile(b)
    r = subprocess.run([exe, "law", a, b, c], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(c, dtype=np.float64).reshape(len(ints), OUT)


def _rot(rpy):
    r, p, y = rpy
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def chain_constants(model):
    """E [dof][9], xyz [dof][3], joint types of a RobotModel: what sai2b_set_collision copies into the law's block"""
    n = int(model.dof)
    E = np.array([_rot(list(model.joint_rpy[i])).reshape(9) for i in range(n)])
    return E, np.array([list(model.joint_xyz[i]) for i in range(n)]), np.array([model.joint_type[i] for i in range(n)])


def _geometry(robot, rng):
    """one random geometry -> (reference, ints prefix [45], constant doubles [163])"""
    m, links, text = cc.model(robot)
    n = int(m.dof)
    names = cc.moving_links(robot)
    S, P, O = int(rng.integers(1, 17)), int(rng.integers(0, 3)), int(rng.integers(0, 5))
    spheres = []
    for _ in range(S):
        l = int(rng.integers(-1, n))
        spheres.append((None, rng.uniform(-0.6, 0.6, 3), rng.uniform(0.0, 0.08)) if l < 0 else (names[l], rng.uniform(-0.1, 0.1, 3), rng.uniform(0.0, 0.08)))
    base = cc.PITCHED_BASE if rng.random() < 1 / 3 else None
    idx, cen, rad = product_spheres(pkg, links, spheres)
    env_mask = int(rng.integers(0, 1 << S))
    pair_mask = [int(rng.integers(0, 1 << S)) & ~((2 << i) - 1) if i < S else 0 for i in range(16)]
    margins = rng.uniform(-0.05, 0.4, 3)
    ref = CollisionReference(text, spheres, P, O, env_mask=env_mask, pair_mask=pair_mask, margins=margins, base=base)
    E, xyz, jt = chain_constants(m if base is None else pkg.with_base_transform(m, base[0], base[1]))
    ints = np.zeros(INTS, dtype=np.int64)
    ints[0:5] = n, S, P, O, env_mask
    ints[5:21] = pair_mask
    ints[21 : 21 + S], ints[21 + S : 37] = idx, -1
    ints[37 : 37 + n] = jt
    v = np.zeros(163)
    v[0 : 9 * n], v[72 : 72 + 3 * n] = E.reshape(-1), xyz.reshape(-1)
    v[96 : 96 + 3 * S], v[144 : 144 + S], v[160:163] = cen.reshape(-1), rad, margins
    return ref, ints, v, (m, n, P, O, S)


def _robots(m, n, P, O, K, rng):
    lo, hi = np.array(m.q_lower[:n]), np.array(m.q_upper[:n])
    q = np.ascontiguousarray((lo + (hi - lo) * rng.uniform(0.05, 0.95, (K, n))).T)
    env = np.zeros((6 * P + 4 * O, K))
    for p in range(P):
        nrm = rng.normal(size=(3, K))
        env[6 * p + 3 : 6 * p + 6] = nrm / np.linalg.norm(nrm, axis=0)
        env[6 * p : 6 * p + 3] = rng.uniform(-0.8, 0.8, (3, K))
    for o in range(O):
        env[6 * P + 4 * o : 6 * P + 4 * o + 3] = rng.uniform(-0.9, 0.9, (3, K))
        env[6 * P + 4 * o + 3] = rng.uniform(0.0, 0.2, K)
    if P + O:
        absent = rng.random(K) < 0.1
        env[rng.integers(0, 6 if P else 4), absent] = np.nan  # somewhere in plane 0, or in obstacle 0 when there is no plane
    bad = rng.random(K) < 0.02
    q[rng.integers(0, n), bad] = rng.choice([np.nan, np.inf, -np.inf])
    return q, env


_recorded = []


def _records():
    """[(robot, ints, values, [(reference outputs, dof, spheres, margins)] per geometry)]: drawn and evaluated once for both builds"""
    if not _recorded:
        rng = np.random.default_rng(20261021)
        for robot in cc.ROBOTS:
            ints, vals, refs = [], [], []
            for _ in range(GEOMETRIES):
                ref, gi, gv, (m, n, P, O, S) = _geometry(robot, rng)
                q, env = _robots(m, n, P, O, PER_GEOMETRY, rng)
                v = np.zeros((PER_GEOMETRY, IN))
                v[:, :163], v[:, 163 : 163 + n], v[:, 171 : 171 + 6 * P + 4 * O] = gv, q.T, env.T
                ints.append(np.tile(gi, (PER_GEOMETRY, 1))), vals.append(v)
                refs.append((ref.evaluate(q, env), n, S, np.array(ref.margins)))
            _recorded.append((robot, np.concatenate(ints), np.concatenate(vals), refs))
    return _recorded


@pytest.mark.parametrize("sanitize", [False, True])
def test_driver_equals_the_restatement(tmp_path_factory, tmp_path, sanitize):
    exe = _build(tmp_path_factory, sanitize)
    worst = dict(distance=0.0, normal=0.0, gradient=0.0, centres=0.0)
    seen_flags, empty = set(), 0
    for robot, ints, vals, refs in _records():
        out = _run(exe, tmp_path, ints, vals)
        assert len(out) == GEOMETRIES * PER_GEOMETRY == 10000
        for g, (ev, n, S, margins) in enumerate(refs):
            o = out[g * PER_GEOMETRY : (g + 1) * PER_GEOMETRY]
            what = (robot, g)
            # the records are well separated: nothing below hangs on a rounding
            assert (ev["gap"] > 1e-9).all() and (ev["norm"] > 1e-3).all(), what
            assert (np.abs(ev["distance"] - margins[:, None]) > 1e-9).all(), what
            assert np.array_equal(o[:, 87].astype(np.uint8), ev["flags"]), what
            # a robot whose q is not finite reports that alone; what its rows hold is not part of the law (0 * inf here, inf there)
            seen_flags |= set(ev["flags"].tolist())
            ok = ev["flags"] != 8
            o = o[ok]
            ev = {k: (v[..., ok] if isinstance(v, np.ndarray) else v) for k, v in ev.items()}
            assert np.array_equal(o[:, 3:6].T, ev["index"]), what
            got = dict(distance=o[:, 0:3].T, normal=o[:, 6:15].T, centres=o[:, 39 : 39 + 3 * S].T,
                       gradient=np.concatenate([o[:, 15 + 8 * c : 15 + 8 * c + n].T for c in range(3)]))
            for k, a in got.items():
                r = ev[k]
                assert np.array_equal(np.isnan(a), np.isnan(r)) and np.array_equal(np.isinf(a), np.isinf(r)), (what, k)
                with np.errstate(invalid="ignore"):
                    err = np.nanmax(np.where(np.isfinite(r), np.abs(a - r), 0.0), initial=0.0)
                worst[k] = max(worst[k], err)
                assert err < TOL, (what, k, err)
            empty += int((ev["index"] < 0).sum())
    print("worst errors:", {k: f"{v:.2e}" for k, v in worst.items()}, "flag bytes seen:", sorted(seen_flags), "empty categories:", empty)
    assert {0, 1, 2, 4, 8} <= seen_flags and empty > 0

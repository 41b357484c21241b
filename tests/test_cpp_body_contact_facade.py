"""The whole-arm contact members of the C++ facade (include/Sai2PrimitivesBatched.h: setBodyContact, clearBodyContact,
getBodyContact, getBodyContactState, robotsTouching on BatchedSimulation; setBodyContact, clearBodyContact, getBodyContactState on
ShardedRobotController), compiled with g++ against the C ABI the way tests/test_cpp_collision_facade.py builds its program
(tests/cpp/body_contact_facade_test.cpp): without a device the members by signature and the exceptions that need no device; on
the GPU 64 Pandas of tests/body_contact_cases.py through six periods of three substeps, planes and obstacles pushing, state,
status and counts after every period equal to the Python mirror's to the bit (one library, one kernel, the same inputs); then the sharded members on two shards of
one device with explicit pairs and every category, status gathered and counts summed, equal to one context's."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")
URDF = os.path.join(ROOT, "tests", "golden", "urdf", "panda_arm.urdf")
PERIODS, SUBSTEPS = 6, 3


@pytest.fixture(scope="module")
def facade_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "body_contact_facade_test")
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "cpp", "body_contact_facade_test.cpp"), "-o", out, "-L", CSRC, "-lsai2b", f"-Wl,-rpath,{CSRC}",
         "-Wl,-rpath,/opt/rocm/lib"],
        check=True,
    )
    return out


def test_cpp_body_contact_members_compile_and_reject_bad_arguments(facade_bin):
    r = subprocess.run([facade_bin, "validate"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and r.stdout.count("ok ") == 12


@pytest.mark.gpu
def test_cpp_body_contact_through_six_periods_equals_the_python_mirror(facade_bin, tmp_path):
    import body_contact_cases as bc
    import sai2_primitives_perso_amd as pkg
    from body_contact_reference import OBSTACLE, PLANE

    case = bc.draw(bc.FACADE_CELL)
    B, n, S, P, O = case["B"], case["n"], len(case["idx"]), case["P"], case["O"]
    cats = PLANE | OBSTACLE  # the facade's geometry has the default pairs, which overlap on the Panda in every posture
    head = np.array([B, S, P, O, cats, bc.V_EPS, PERIODS, SUBSTEPS], dtype=np.float64)
    parts = [head, case["q"], case["dq"], case["tau"], case["idx"].astype(np.float64), case["cen"], case["rad"], case["env"], case["rows"]]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.ascontiguousarray(p, dtype=np.float64).reshape(-1) for p in parts]).tofile(fin)
    r = subprocess.run([facade_bin, "run", URDF, fin, fout], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "0 failures" in r.stdout and "FAILED" not in r.stdout
    per, per_sharded = 2 * n * B + (9 + n) * B + 4, (9 + n) * B + 4
    raw = np.fromfile(fout, dtype=np.float64)
    assert raw.size == PERIODS * per + 2 * per_sharded
    got, got_sharded = raw[: PERIODS * per].reshape(PERIODS, per), raw[PERIODS * per :].reshape(2, per_sharded)
    # the Python mirror on the same inputs
    model, _ = pkg.model_from_urdf(URDF)
    g = pkg.Controller(model, [pkg.motion_force_task_config("m", link=n - 1, frame_pos=(0.0, 0.0, 0.15), robot_dof=n), pkg.joint_task_config("j", robot_dof=n)], B)
    g.set_state(case["q"], case["dq"])
    g.set_collision(g.collision_config(case["idx"], case["cen"], case["rad"], n_planes=P, n_obstacles=O), case["env"])
    g.set_body_contact(case["rows"], categories=("plane", "obstacle"), v_eps=bc.V_EPS)
    touched = 0
    for p in range(PERIODS):
        g.sim_step(case["tau"], 1e-3, SUBSTEPS, False)
        q, dq = g.get_state()
        st = g.get_body_contact_state()
        want = np.concatenate([q.reshape(-1), dq.reshape(-1), st["status"].reshape(-1), [st["counts"][k] for k in ("plane", "obstacle", "self", "any")]])
        assert np.array_equal(got[p], want), p
        touched = max(touched, st["counts"]["any"])
    assert touched >= B // 4
    # the sharded members: two shards, explicit pairs, every category; robot by robot the single context's results
    g.set_state(case["q"], case["dq"])
    g.set_collision(g.collision_config(case["idx"], case["cen"], case["rad"], n_planes=P, n_obstacles=O, pairs=bc.pairs("panda")), case["env"])
    g.set_body_contact(case["rows"], v_eps=bc.V_EPS)
    selfs = 0
    for p in range(2):
        g.sim_step(case["tau"], 1e-3, SUBSTEPS, False)
        st = g.get_body_contact_state()
        want = np.concatenate([st["status"].reshape(-1), [st["counts"][k] for k in ("plane", "obstacle", "self", "any")]])
        assert np.array_equal(got_sharded[p], want), p
        selfs = max(selfs, st["counts"]["self"])
    assert selfs > 0

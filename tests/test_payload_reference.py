"""Per-robot payloads without a GPU: the yardstick of tests/test_gpu_payload.py (the C oracle on the URDF text with the payload
as a fixed-joint body) against the 40-digit model of tests/hp_reference.py, the sensitivity of the torques to the payloads, the
C ABI and the C++ facade, and the gfx950 code of the headline kernel's payload form."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hp_dynamics_fixture as hd
import hp_reference as hp
import oracle_lib as ol
import payload_cases as pc
import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EPS = hd.EPS
POSES = 8


def test_the_fixture_has_the_payloads_it_must_have():
    m, c, I = pc.payloads()
    assert m[0] == 0 and not I[:, 0].any()
    assert m[1] == 3.0 and np.hypot(c[0, 1], c[1, 1]) == 0.2 and not I[:, 1].any()
    assert (I[3:, 2] != 0).all() and m[3] == 0.05
    assert ((m[4:] >= 0.1) & (m[4:] <= 3)).all() and (np.linalg.norm(c[:, 4:], axis=0) <= 0.15).all() and np.abs(I[:, 4:]).max() <= 0.05
    for k in range(pc.P):  # positive semi-definite about the COM
        S = np.array([[I[0, k], I[3, k], I[4, k]], [I[3, k], I[1, k], I[5, k]], [I[4, k], I[5, k], I[2, k]]])
        assert np.linalg.eigvalsh(S).min() >= -1e-18
    mm, _, _ = pc.rows(70)
    assert (mm[1:] != mm[:-1]).all()  # neighbouring lanes always differ


@pytest.mark.parametrize("k", range(pc.P))
def test_the_oracle_on_the_merged_model_meets_the_40_digit_sum_over_bodies(k):
    """M, g and the bias vector for 8 poses. Bounds: the bias and gravity vectors to C_BIAS eps beta (tests/hp_dynamics_fixture.py,
    beta from hp.bias_terms: the payload is one more body in the same sums); M, a sum of n + 1 bodies' m Jv^T Jv + Jw^T I Jw
    whose terms are products of a few rounded factors, to C_BIAS eps max|M|."""
    text = pc.texts("panda")[k]
    model = hp.Model(text)
    pm, _ = pkg.model_from_urdf(text, is_file=False)
    rng = np.random.default_rng(100 + k)
    q = np.ascontiguousarray(rng.uniform(-1.2, 1.2, size=(7, POSES)))
    q[3] = -1.5 + 0.5 * q[3]
    dq = np.ascontiguousarray(rng.uniform(-1, 1, size=(7, POSES)))
    o = ol.Oracle(pm, [ol.joint_task("j")], POSES)
    o.set_state(q, dq)
    o.enable_gravity_compensation(True)
    o.tick()
    M, g, b0, bg = o.get_model(), o.get_gravity(), o.get_bias(False), o.get_bias(True)
    for p in range(POSES):
        _, _, Mx, gx = model.dynamics(q[:, p])
        Mx = np.array([[float(Mx[i, j]) for j in range(7)] for i in range(7)])
        assert np.abs(M[:, p].reshape(7, 7) - Mx).max() <= hd.C_BIAS * EPS * np.abs(Mx).max(), (k, p)
        bx, beta = hp.bias_terms(model, q[:, p], dq[:, p], None)
        bx, beta = np.array([float(x) for x in bx]), float(hp.norm_inf(beta))
        assert np.abs(bg[:, p] - bx).max() <= hd.C_BIAS * EPS * beta, (k, p)
        assert np.abs(g[:, p] - np.array([float(x) for x in gx])).max() <= hd.C_BIAS * EPS * beta, (k, p)
        b0x, beta0 = hp.bias_terms(model, q[:, p], dq[:, p], False)
        assert np.abs(b0[:, p] - np.array([float(x) for x in b0x])).max() <= hd.C_BIAS * EPS * max(float(hp.norm_inf(beta0)), 1e-300), (k, p)


def test_torques_move_by_far_more_than_the_parity_tolerance():
    """C3 workload: with payload j against no payload, every robot whose payload is at least 0.5 kg: more than 1000 x the
    parity tolerance (1e-10) relative to max|tau|"""
    B = 512
    inp = pkg.workloads.make_inputs(3, B=B)
    cfgs = ol.task_configs(inp["tasks"])
    o = pc.PayloadOracles(pc.texts("panda"), cfgs, B)
    o0 = ol.Oracle(pkg.model_from_urdf(pc.texts("panda")[0], is_file=False)[0], cfgs, B, threads=8)
    for c in (o, o0):
        c.load_inputs(inp) if c is o else ol.load_inputs(c, inp)
        c.enable_gravity_compensation(True)
    tau, tau0 = o.tick(), o0.tick()
    m, _, _ = pc.rows(B)
    d = np.abs(tau - tau0).max(axis=0) / np.abs(tau0).max()
    assert (m >= 0.5).sum() > B // 2
    assert d[m >= 0.5].min() > 1000 * 1e-10, d[m >= 0.5].min()
    assert np.array_equal(tau[:, m == 0], tau0[:, m == 0])


@pytest.mark.parametrize("cell", list(pc.HP_CELLS))
def test_the_oracle_on_the_urdf_text_meets_the_blending_region_fixture(cell):
    """tests/golden/hp_payload.npz: the oracle on the merged model within the bound of tests/test_hp_reference.py (C_TICK eps
    kappa_emp), its bookkeeping the fixture's; the fixture is small"""
    import hp_fixture as hf

    assert os.path.getsize(pc.HP_FIXTURE) < 200_000
    d = pc.hp_load(cell)
    B = d["dq"].shape[1]
    assert B == pc.HP_CELLS[cell] and sum(pc.HP_CELLS.values()) == 32
    tau = np.empty_like(d["tau"][0])
    n = np.empty(B, dtype=int)
    for k, text in enumerate(pc.hp_texts(cell)):
        sel = np.arange(k, B, len(pc.HP_PAYLOADS))
        model, _ = pkg.model_from_urdf(text, is_file=False)
        sub = {key: (v[..., sel] if v.ndim and v.shape[-1] == B else v) for key, v in d.items()}
        o = pc.hp_make(cell, sub, ol.joint_task, ol.motion_force_task, lambda m, cfgs, b: ol.Oracle(m, cfgs, b), model=model)
        (t, state), = hf.run(o, cell, sub)
        tau[:, sel], n[sel] = t, state[0]
    r = hf.ratio_to_bound(tau, d, 0)
    assert r.max() <= hd.C_TICK, (cell, r.max())
    assert np.array_equal(n, d["nsing"][0].astype(int))


def test_abi_exports_and_the_cpp_facade(tmp_path):
    lib = _abi.load_library()
    for sym in ("sai2b_set_link_payload", "sai2b_clear_link_payload", "sai2b_get_link_payload"):
        assert sym in _abi.EXPORTS and getattr(lib, sym)
    header = open(os.path.join(ROOT, "include", "sai2b.h")).read()
    assert re.search(r"SAI2B_BUF_PAYLOAD\s*=\s*%d\b" % _abi.BUF_PAYLOAD, header)
    assert re.search(r"SAI2B_BUF_PLANT_PAYLOAD\s*=\s*%d\b" % _abi.BUF_PLANT_PAYLOAD, header)
    for name, v in (("CONTROLLER", 1), ("PLANT", 2), ("BOTH", 3)):
        assert re.search(r"SAI2B_PAYLOAD_%s\s*=\s*%d\b" % (name, v), header) and _abi.PAYLOAD_TARGETS[name.lower()] == v
    # a null context is refused, not dereferenced
    assert lib.sai2b_set_link_payload(None, 3, 0, None, None, None, 0) != 0
    src = tmp_path / "payload_facade.cpp"
    src.write_text('''#include "Sai2PrimitivesBatched.h"
int main(int argc, char**) {
	if (argc < 100) return 0;  // compiled and linked, never run here (no device)
	Sai2Primitives::BatchedRobotModel robot(64);
	Sai2Primitives::Batch mass(64, 1.0), com(3 * 64, 0.01), inertia(6 * 64, 0.0);
	robot.setLinkPayload(6, mass);
	robot.setLinkPayload(6, mass, com, inertia, SAI2B_PAYLOAD_PLANT);
	const double pos[3] = {0, 0, 0.1};
	robot.setLinkPayload("link7", pos, nullptr, mass, com, inertia);
	robot.clearLinkPayload(SAI2B_PAYLOAD_CONTROLLER);
	robot.clearLinkPayload();
	return 0;
}
''')
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "payload_facade"),
                    "-L", CSRC, "-lsai2b", "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"], check=True)
    subprocess.run([str(tmp_path / "payload_facade")], check=True)

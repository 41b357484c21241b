"""CPU check of the Panda model functions written out from the model's nonzero terms (csrc/tools/gen_baked_model.cpp ->
csrc/sai2b_baked_panda_model.h, what the baked kernels run): tests/cpp/baked_model_driver.cpp evaluates them on the host
next to the generic formulas on the same constants.

500 random poses inside the joint limits, both limits and q = 0. Control-point pose, Jacobian, M and g (and M, g with a
payload on link 3, the forms with the payload selects):
  * written out against generic: every entry within 64 eps of the quantity's largest entry. Dropping a term whose
    factor is exactly 0 and turning a factor 1 into a copy change no rounding; what differs is the composite inertia of
    the isotropic links (s added to the diagonal instead of R (s 1) R^T, equal only as far as R R^T = 1 is) and how the
    compiler contracts a * b + c. The generic M itself is some 30 roundings deep;
  * written out against tests/urdf_np.py (xml.etree + the URDF's own semantics + numpy) at the 1e-12 (M, g) and 1e-13
    (J, x, R) of tests/test_urdf.py.
The driver runs once more as a stand-alone program built with -fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

import hp_fixture
import sai2_primitives_perso_amd as pkg
import urdf_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "cpp", "baked_model_driver.cpp")
EPS = np.finfo(float).eps
FRAME = ("end-effector", (0.01, -0.02, 0.07))
PAYLOAD_LINK = 3
SIZES = [("x", 3), ("R", 9), ("J", 42), ("M", 49), ("g", 7), ("M_payload", 49), ("g_payload", 7)]


def _build(tmp_path, name, *flags):
    if not os.path.exists(os.path.join(CSRC, "sai2b_baked_panda_model.h")):  # generated header (build() makes it too)
        subprocess.run(["make", "-C", CSRC, "sai2b_baked_panda.h"], check=True)
    out = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", *flags, "-I", CSRC, DRIVER, "-o", out], check=True)
    return out


def _poses():
    m = pkg.panda_model()
    lo, hi = np.array(list(m.q_lower)[:7]), np.array(list(m.q_upper)[:7])
    rng = np.random.default_rng(11)
    q = lo[:, None] + (hi - lo)[:, None] * rng.uniform(0, 1, (7, 500))
    return np.concatenate([q, lo[:, None], hi[:, None], np.zeros((7, 1))], axis=1)


def _run(exe, tmp_path, q, link, fpos):
    path = str(tmp_path / "poses.txt")
    with open(path, "w") as f:
        f.write(f"{link} {float(fpos[0])!r} {float(fpos[1])!r} {float(fpos[2])!r} {PAYLOAD_LINK}\n")
        for b in range(q.shape[1]):
            f.write(" ".join(repr(float(v)) for v in q[:, b]) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    rows = {"S": [], "G": []}
    for line in r.stdout.splitlines():
        tag, *vals = line.split()
        rows[tag].append([float.fromhex(v) for v in vals])
    out = {}
    for tag, a in rows.items():
        a = np.array(a)
        assert a.shape == (q.shape[1], sum(n for _, n in SIZES)), a.shape
        cuts = np.cumsum([0] + [n for _, n in SIZES])
        out[tag] = {name: a[:, cuts[i]:cuts[i + 1]] for i, (name, _) in enumerate(SIZES)}
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("baked_model")
    text = hp_fixture.urdf_text("panda")
    model, links = pkg.model_from_urdf(text, is_file=False)
    assert bytes(model) == bytes(pkg.panda_model()), "the URDF is the baked model's"
    link, fpos, frot = pkg.resolve_link_frame(links, *FRAME)
    q = _poses()
    return q, np.asarray(frot, dtype=float).reshape(3, 3), _run(_build(tmp, "baked_model_driver"), tmp, q, link, fpos), (link, fpos)


def test_written_out_functions_equal_the_generic_ones_to_rounding(results):
    q, _, out, _ = results
    for name, _ in SIZES:
        s, g = out["S"][name], out["G"][name]
        assert np.isfinite(s).all() and np.isfinite(g).all()
        rel = np.abs(s - g).max(axis=1) / np.abs(g).max(axis=1)
        print(f"{name}: largest difference written out vs generic {rel.max() / EPS:.1f} eps of the largest entry (pose {int(rel.argmax())})")
        assert rel.max() <= 64 * EPS, (name, int(rel.argmax()), rel.max() / EPS)


def test_written_out_functions_match_an_independent_reading_of_the_urdf(results):
    q, frot, out, _ = results
    ch = urdf_np.Chain(hp_fixture.urdf_text("panda"), is_file=False)
    s = out["S"]
    worst = dict.fromkeys(("M", "g", "J", "x", "R"), 0.0)
    for b in range(q.shape[1]):
        Mn, gn = ch.mass_matrix_and_gravity(q[:, b])
        Jn, xn, Rn = ch.jacobian(q[:, b], *FRAME)
        err = {"M": np.abs(s["M"][b].reshape(7, 7) - Mn).max() / max(1.0, np.abs(Mn).max()),
               "g": np.abs(s["g"][b] - gn).max() / max(1.0, np.abs(gn).max()),
               "J": np.abs(s["J"][b].reshape(6, 7) - Jn).max(), "x": np.abs(s["x"][b] - xn).max(),
               "R": np.abs(s["R"][b].reshape(3, 3) @ frot - Rn).max()}
        worst = {k: max(worst[k], err[k]) for k in worst}
    print("largest difference to urdf_np:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["M"] < 1e-12 and worst["g"] < 1e-12, worst
    assert worst["J"] < 1e-13 and worst["x"] < 1e-13 and worst["R"] < 1e-13, worst


def test_driver_is_clean_under_address_and_undefined_sanitizers(results, tmp_path):
    q, _, out, (link, fpos) = results
    exe = _build(tmp_path, "baked_model_driver_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    again = _run(exe, tmp_path, q[:, -8:], link, fpos)
    for name, _ in SIZES:
        assert np.allclose(again["S"][name], out["S"][name][-8:], rtol=0, atol=1e-12)

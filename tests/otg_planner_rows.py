"""Input rows for the planner tests of tests/test_gpu_otg_planner.py, the harness that runs them
(tests/cpp/otg_planner_device.hip) and the reference's ruckig run on the same rows.

A batch is (n [R] int32, X [R, 8, 8] float64, frac [R, 6]): X[r, k] is cp, cv, ca, tp, tv, vmax, amax, jmax for k = 0..7,
lanes j >= n[r] are padding. Every family is seeded and is drawn for n = 1 .. nmax."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "sai2-primitives-perso_amd", "csrc")
HARNESS = os.path.join(HERE, "cpp", "otg_planner_device.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_otg_golden as mog  # noqa: E402
import otg_np  # noqa: E402

W, NF, NT = 8, 6, 8
EPS = np.finfo(float).eps
CP, CV, CA, TP, TV, VM, AM, JM = range(8)
PATHS = {"host_acc": 0, "host_jerk": 1, "group_acc": 2, "group_jerk": 3, "lane_acc": 4, "lane_jerk": 5}
ERR_TRAJECTORY_DURATION = -101


def hipcc_flags(n_joints):
    """csrc/Makefile's flags for sai2b_otg_n*.o (the 8-joint build's generators take SAI2B_OTG_MAXD = 8 from the file)"""
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", f"-DSAI2B_N={n_joints}", "-I", CSRC,
            "-include", "sai2b_dof_rename.h"]


def build_harness(n_joints, out, timeout=300):
    subprocess.run([HIPCC, *hipcc_flags(n_joints), "-fPIC", "-shared", HARNESS, "-o", out], check=True, timeout=timeout)
    L = C.CDLL(out)
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.otgh_run.argtypes = [C.c_int, C.c_int, ip, dp, dp, ip, dp, ip, dp, dp, dp]
    L.otgh_stepped.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, ip, dp, dp, dp, dp, ip, dp, ip]
    return L


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def run(L, path, n, X, frac):
    """one harness path over a batch -> dict res, dur, meta [R,3,8], bdur [R,8], tph [R,8,7], pva [R,3,NT,8]"""
    R = len(n)
    n, X, frac = (np.ascontiguousarray(a, dtype=t) for a, t in ((n, np.int32), (X, float), (frac, float)))
    o = {"res": np.zeros(R, np.int32), "dur": np.zeros(R), "meta": np.zeros((R, 3, W), np.int32), "bdur": np.zeros((R, W)),
         "tph": np.zeros((R, W, 7)), "pva": np.zeros((R, 3, NT, W))}
    err = L.otgh_run(PATHS[path], R, _ptr(n, C.c_int), _ptr(X, C.c_double), _ptr(frac, C.c_double), _ptr(o["res"], C.c_int),
                     _ptr(o["dur"], C.c_double), _ptr(o["meta"], C.c_int), _ptr(o["bdur"], C.c_double), _ptr(o["tph"], C.c_double),
                     _ptr(o["pva"], C.c_double))
    assert err == 0, (path, err)
    return o


def reference(ref, jerk, n, X, frac):
    """ruckig's answers (rref_calculate_and_sample[_jerk]) -> res, dur, pva [R,3,NT,8], as ruckig_record.calc3 samples"""
    R = len(n)
    X = np.ascontiguousarray(X, dtype=float)
    fn = ref.rref_calculate_and_sample_jerk if jerk else ref.rref_calculate_and_sample
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * (8 if jerk else 7) + [C.POINTER(C.c_double), C.c_int] + [C.c_void_p] * 4
    res, dur, pva = np.zeros(R, np.int32), np.zeros(R), np.zeros((R, 3, NT, W))
    base, d = X.ctypes.data, C.c_double()
    bufs = [np.zeros(NT * W) for _ in range(3)]
    times = np.zeros(NT)
    keys = range(8) if jerk else range(7)
    for r in range(R):
        k = int(n[r])
        args = [base + (r * W + q) * W * 8 for q in keys]
        rr = fn(k, otg_np.SYNC_PHASE, *args, C.byref(d), 0, times.ctypes.data, *(b.ctypes.data for b in bufs))
        T = d.value
        if rr == 0:
            times[:NF] = frac[r] * T
            times[NF], times[NF + 1] = T, T + 0.01
            rr = fn(k, otg_np.SYNC_PHASE, *args, C.byref(d), NT, times.ctypes.data, *(b.ctypes.data for b in bufs))
            for q in range(3):
                pva[r, q, :, :k] = bufs[q][: NT * k].reshape(NT, k)
        res[r], dur[r] = rr, T
    return {"res": res, "dur": dur, "pva": pva}


# ---- input families ----
class Rows:
    def __init__(self):
        self.n, self.X, self.frac, self.fam = [], [], [], []

    def add(self, fam, n, cp, cv, ca, tp, tv, vm, am, jm, frac):
        x = np.zeros((W, W))
        for q, v in enumerate((cp, cv, ca, tp, tv, vm, am, jm)):
            x[q, :n] = np.asarray(v, dtype=float)[:n]
        self.n.append(n), self.X.append(x), self.frac.append(np.asarray(frac, dtype=float)), self.fam.append(fam)

    def arrays(self):
        return np.array(self.n, np.int32), np.array(self.X), np.array(self.frac), np.array(self.fam)


def _frac(rng):
    return np.sort(rng.uniform(0, 1, NF))


def _limits(rng, n, lo=0.08, hi=16.0):
    return rng.uniform(lo, hi, n), rng.uniform(lo, hi, n), rng.uniform(0.5, 40, n)


def _blocked_pairs(ref, rng, count=3000):
    """2-DoF inputs whose synchronised duration (ruckig, either planner) exceeds both DoFs' own minimum durations:
    a blocked interval of one DoF decides it. About 2 % of these draws do. -> [k][8 quantities][2 DoFs]"""
    rows = Rows()
    for _ in range(count):
        vm, am, jm = _limits(rng, 2, 0.3, 4.0)
        cp, ca = np.zeros(2), np.zeros(2)
        tp = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-3, 3)])
        cv, tv = rng.uniform(-1, 1, 2) * vm, rng.uniform(-1, 1, 2) * vm
        fr = _frac(rng)
        rows.add("pair", 2, cp, cv, ca, tp, tv, vm, am, jm, fr)
        for d in range(2):
            rows.add("single", 1, cp[d:], cv[d:], ca[d:], tp[d:], tv[d:], vm[d:], am[d:], jm[d:], fr)
    n, X, frac, fam = rows.arrays()
    hit = np.zeros(count, bool)
    for jerk in (False, True):
        rf = reference(ref, jerk, n, X, frac)
        d, r = rf["dur"].reshape(count, 3), rf["res"].reshape(count, 3)
        hit |= (r == 0).all(1) & (d[:, 0] > np.maximum(d[:, 1], d[:, 2]) * (1 + 1e-9) + 1e-12)
    return X[::3][hit][:, :, :2]


def families(nmax, ref, seed=0):
    """the rows of every family for generators of 1 .. nmax DoFs -> (n, X, frac, family name per row); `ref` (the
    reference's ruckig) picks the rows of the blocked-interval family"""
    rng = np.random.default_rng(1000 + seed + nmax)
    out = Rows()
    pairs = _blocked_pairs(ref, rng)
    # ruckig-style random rows (make_otg_golden.random_calc_inputs; jerk as ruckig_record.otg3_random)
    for row in mog.random_calc_inputs(1400 * nmax // 7, seed=4000 + nmax, nmax=nmax, maxd=W):
        n, sync, cp, cv, ca, tp, tv, vm, am, frac = row
        if sync == otg_np.SYNC_PHASE:
            out.add("random", n, cp, cv, ca, tp, tv, vm, am, rng.uniform(0.5, 40, n), frac)
    for n in range(1, nmax + 1):
        for it in range(60):
            # brake pre-trajectories: |cv| above vmax, |ca| above amax (the jerk-limited planner brakes on both)
            vm, am, jm = _limits(rng, n)
            s = np.sign(rng.normal(size=n))
            cv = s * vm * rng.uniform(1.0001, 3, n) * (rng.random(n) < 0.7)
            ca = np.sign(rng.normal(size=n)) * am * rng.uniform(1.0001, 3, n) * (rng.random(n) < 0.5)
            if it % 3 == 0:
                ca = rng.normal(0, 0.5, n)
            cp, tp = rng.normal(0, 2, n), rng.normal(0, 2, n)
            tv = np.where(rng.random(n) < 0.3, rng.uniform(-1, 1, n) * vm, 0.0)
            out.add("brake", n, cp, cv, ca, tp, tv, vm, am, jm, _frac(rng))
        for it in range(60):
            # non-zero target velocities, some exactly +-vmax
            vm, am, jm = _limits(rng, n)
            tv = rng.uniform(-1, 1, n) * vm
            edge = rng.random(n) < 0.3
            tv[edge] = np.sign(rng.normal(size=edge.sum())) * vm[edge]
            cv = np.where(rng.random(n) < 0.6, rng.uniform(-1, 1, n) * vm, 0.0)
            ca = np.where(rng.random(n) < 0.4, rng.normal(0, 1, n), 0.0)
            cp = rng.normal(0, 1, n)
            tp = cp + rng.normal(0, 0.3, n) * (10.0 ** rng.uniform(-3, 1, n))
            out.add("target_velocity", n, cp, cv, ca, tp, tv, vm, am, jm, _frac(rng))
        if n > 1:
            # a blocked interval decides the duration: two DoFs that do (found by _blocked_pairs), the others moving a
            # little from rest, in random lanes; each DoF follows again as its own n = 1 row
            for it in range(len(pairs) // (nmax - 1)):
                a = pairs[(n - 2) * (len(pairs) // (nmax - 1)) + it]
                vm, am, jm = _limits(rng, n)
                cp = rng.normal(0, 1, n)
                tp = cp + rng.normal(0, 1e-3, n)
                cv, ca, tv = np.zeros(n), np.zeros(n), np.zeros(n)
                lanes = rng.permutation(n)[:2]
                for q, v in enumerate((cp, cv, ca, tp, tv, vm, am, jm)):
                    v[lanes] = a[q]
                fr = _frac(rng)
                out.add("blocked", n, cp, cv, ca, tp, tv, vm, am, jm, fr)
                for d in range(n):
                    out.add("blocked_single", 1, cp[d:], cv[d:], ca[d:], tp[d:], tv[d:], vm[d:], am[d:], jm[d:], fr)
        if n > 1:
            for it in range(48):
                # collinear rows (phase synchronisation), dyadic so that the scaled differences are exact, and the same
                # rows just off collinear: 0.5, 1, 2 x EPS in one component
                vm, am, jm = _limits(rng, n)
                dvec = rng.integers(-8, 9, n) / 8.0
                dvec[0] = dvec[0] or 0.5
                if it % 4 == 3:
                    dvec[rng.integers(1, n)] = 0.0
                s = 2.0 ** rng.integers(-3, 3)
                cp = rng.integers(-64, 64, n) / 16.0
                tp = cp + dvec * s
                k_v, k_a, k_t = (2.0 ** rng.integers(-4, 1) * rng.integers(-2, 3) for _ in range(3))
                cv, ca, tv = dvec * k_v, dvec * k_a * (it % 2), dvec * k_t * (it % 3 == 0)
                vm = np.maximum(vm, np.abs(tv) * 1.5)
                fr = _frac(rng)
                out.add("collinear", n, cp, cv, ca, tp, tv, vm, am, jm, fr)
                if it % 2 == 0:  # ruckig's own kind: float scale
                    d2 = rng.normal(0, 1, n)
                    c2 = rng.normal(0, 2, n)
                    out.add("collinear", n, c2, d2 * rng.normal(0, 0.3), d2 * 0, c2 + d2 * rng.uniform(0.1, 3), d2 * 0, vm, am, jm, fr)
                for m in (0.5, 1.0, 2.0):
                    q = (CV, CA, TV, TP)[it % 4]
                    vals = [cp.copy(), cv.copy(), ca.copy(), tp.copy(), tv.copy()]
                    j = int(rng.integers(0, n))
                    vals[q][j] += m * EPS * (1 if vals[q][j] == 0 else abs(vals[q][j]))
                    out.add("near_collinear", n, *vals, vm, am, jm, fr)
        for it in range(20):
            # at the target: duration 0; one DoF at its target while the others move
            vm, am, jm = _limits(rng, n)
            cp = rng.normal(0, 1, n)
            z = np.zeros(n)
            out.add("at_target", n, cp, z, z, cp, z, vm, am, jm, _frac(rng))
            tp = cp + rng.normal(0, 1, n)
            j = int(rng.integers(0, n))
            tp[j] = cp[j]
            cv = np.where(rng.random(n) < 0.5, rng.normal(0, 0.3, n), 0.0)
            cv[j] = 0
            out.add("at_target", n, cp, cv, z, tp, z, vm, am, jm, _frac(rng))
        if n > 1:
            for it in range(30):
                # exact ties: duplicated DoFs, mirrored DoFs, limits shared by lanes 0-2 and 3-5
                vm, am, jm = _limits(rng, n)
                cp, tp = rng.normal(0, 1, n), rng.normal(0, 1, n)
                cv = np.where(rng.random(n) < 0.5, rng.normal(0, 0.5, n), 0.0)
                ca = np.where(rng.random(n) < 0.3, rng.normal(0, 0.5, n), 0.0)
                tv = np.where(rng.random(n) < 0.3, rng.uniform(-0.5, 0.5, n) * vm, 0.0)
                vals = [cp, cv, ca, tp, tv, vm, am, jm]
                a, b = 0, int(rng.integers(1, n))
                kind = it % 3
                if kind == 0:  # duplicate
                    for v in vals:
                        v[b] = v[a]
                elif kind == 1:  # mirror: same |dp|, opposite sign
                    for v in vals[:5]:
                        v[b] = -v[a]
                    for v in vals[5:]:
                        v[b] = v[a]
                else:  # Cartesian-style limits
                    for v in vals[5:]:
                        v[: min(n, 3)] = v[0]
                        if n > 3:
                            v[3: min(n, 6)] = v[3]
                    vals[1][:] = 0
                    vals[2][:] = 0
                    vals[4][:] = 0
                out.add("ties", n, *vals, _frac(rng))
        for it in range(12):
            # durations near the 7.6e3 s limit: the limiting DoF rest to rest, on either side
            vm, am, jm = _limits(rng, n)
            cp, tp = rng.normal(0, 1, n), rng.normal(0, 1, n)
            z = np.zeros(n)
            v0, a0 = rng.uniform(0.08, 0.2), rng.uniform(0.5, 2)
            j0 = max(a0 * a0 / v0 * rng.uniform(1.5, 4), 1.0)
            rel = (-1e-3, -1e-7, -1e-10, 1e-10, 1e-7, 1e-3)[it % 6]
            Tt = 7.6e3 * (1 + rel)
            d0 = v0 * (Tt - v0 / a0 - (a0 / j0 if it >= 6 else 0.0))
            vm[0], am[0], jm[0] = v0, a0, j0
            tp[0] = cp[0] + d0 * (1 if it % 2 else -1)
            out.add("long", n, cp, z, z, tp, z, vm, am, jm, _frac(rng))
        for it in range(24):
            # tiny displacements, wide limits, jerk from 1e-1 to 1e6
            vm, am = 10.0 ** rng.uniform(np.log10(0.08), np.log10(16), n), 10.0 ** rng.uniform(np.log10(0.08), np.log10(16), n)
            jm = 10.0 ** rng.uniform(-1, 6, n)
            cp = rng.normal(0, 1, n)
            tp = cp + np.sign(rng.normal(size=n)) * 10.0 ** rng.uniform(-12, -6, n)
            z = np.zeros(n)
            cv = z if it % 2 else np.where(rng.random(n) < 0.5, 10.0 ** rng.uniform(-12, -6, n), 0.0)
            out.add("tiny", n, cp, cv, z, tp, z, vm, am, jm, _frac(rng))
    return out.arrays()


def coverage(n, fam, host, ref_single=None):
    """counts of the branches the families are meant to reach, from the host path's outputs (bit-equal to ruckig)"""
    R = len(n)
    act = np.arange(W)[None, :] < n[:, None]
    ok = host["res"] == 0
    brake = ok & ((host["bdur"] > 0) & act).any(1)
    tph = host["tph"]
    same = np.all((tph == tph[:, :1, :]) | ~act[:, :, None], axis=(1, 2))
    phase = ok & (n > 1) & (host["dur"] > 0) & same
    long_err = host["res"] == ERR_TRAJECTORY_DURATION
    out = {"rows": R, "brake": int(brake.sum()), "phase_synced": int(phase.sum()), "err_duration": int(long_err.sum())}
    if ref_single is not None:
        out["blocked"] = int(ref_single.sum())
    return out


def blocked_rows(n, fam, dur, res):
    """rows of the `blocked` family whose synchronised duration exceeds every DoF's own minimum (its n = 1 row, which
    follows it): a blocked interval decided the duration"""
    out = np.zeros(len(n), bool)
    r = 0
    while r < len(n):
        if fam[r] == "blocked" and n[r] > 1:
            k = int(n[r])
            singles = dur[r + 1: r + 1 + k]
            assert (fam[r + 1: r + 1 + k] == "blocked_single").all()
            if res[r] == 0 and (res[r + 1: r + 1 + k] == 0).all() and dur[r] > singles.max() * (1 + 1e-9) + 1e-12:
                out[r] = True
            r += 1 + k
        else:
            r += 1
    return out

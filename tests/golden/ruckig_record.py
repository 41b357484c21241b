"""Recorded answers of the reference's own ruckig (oracle/_ref/libruckig_ref.so) for the bit-for-bit planner tests
(tests/test_otg_core.py, test_otg3_core.py, test_otg_oracle.py), so that they run where that library cannot be built.

Every comparison those tests make is an OBSERVATION: the result code, duration and sampled states of one planner call,
or the output of one stepped Ruckig::update. Each observation is stored as a 16-byte BLAKE2b digest of its float64
bytes (ruckig_recorded.npz), which keeps the comparison bit for bit in a fixture of a few hundred kB. The input draws
live here once, shared by the recording (`python tests/golden/ruckig_record.py` after `make -C oracle ref`) and the
tests, so both see the same inputs. `python tests/golden/ruckig_record.py --append` records only the sequences the
fixture does not hold yet.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_otg_golden as mog  # noqa: E402
import otg_np  # noqa: E402

FIXTURE = os.path.join(HERE, "ruckig_recorded.npz")
dp = C.POINTER(C.c_double)


def digest(*items):
    h = hashlib.blake2b(digest_size=16)
    for x in items:
        h.update(np.ascontiguousarray(np.asarray(x, dtype=np.float64)).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def recorded(name):
    """the digests recorded from the reference for one observation sequence, [k][16] uint8"""
    with np.load(FIXTURE) as z:
        return z[name]


def assert_matches(name, seq):
    """the product's observations (result, digest) against the recorded ones, one by one -> the result codes"""
    want = recorded(name)
    codes = []
    for i, (r, d) in enumerate(seq):
        assert i < len(want) and np.array_equal(d, want[i]), (name, i, r)
        codes.append(r)
    assert len(codes) == len(want), (name, len(codes), len(want))
    return codes


def _P(a):
    return np.ascontiguousarray(a, dtype=float).ctypes.data_as(dp)


def calc3(fn, row, jm):
    """one jerk-limited *_calculate_and_sample call -> (result, duration, positions, velocities, accelerations)"""
    n, sync, cp, cv, ca, tp, tv, vm, am, frac = row
    keep = [np.ascontiguousarray(a[:n]) for a in (cp, cv, ca, tp, tv, vm, am, jm)]
    d = C.c_double()
    fn.restype = C.c_int
    args = [a.ctypes.data_as(dp) for a in keep]
    z = np.zeros(1).ctypes.data_as(dp)
    r = fn(n, sync, *args, C.byref(d), 0, z, z, z, z)
    T = d.value
    times = np.ascontiguousarray(np.concatenate([frac * T, [T, T + 0.01]]))
    op, ov, oa = (np.zeros((len(times), n)) for _ in range(3))
    if r == 0:
        r = fn(n, sync, *args, C.byref(d), len(times), times.ctypes.data_as(dp), op.ctypes.data_as(dp), ov.ctypes.data_as(dp), oa.ctypes.data_as(dp))
    return r, T, op, ov, oa


# ---- observation sequences: each yields (result code, digest) per observation
def otg3_random(fn, n_cases=6000):
    """jerk-limited one-shot calculations on ruckig-style random inputs (phase-synchronised rows)"""
    rng = np.random.default_rng(5)
    for row in mog.random_calc_inputs(n_cases, seed=11):
        if row[1] != otg_np.SYNC_PHASE:  # the wrappers always ask for Synchronization::Phase (OTG_joints.cpp:23)
            continue
        n = row[0]
        jm = np.concatenate([rng.uniform(0.5, 40, n), np.zeros(mog.MAXD - n)])
        out = calc3(fn, row, jm)
        yield out[0], digest(*out)


def otg3_random8(fn, n_cases=8000):
    """otg3_random for the 8-DoF generators of the 8-joint build (SAI2B_OTG_MAXD = 8): the rows with n = 8"""
    rng = np.random.default_rng(55)
    for row in mog.random_calc_inputs(n_cases, seed=811, nmax=8, maxd=8):
        if row[1] != otg_np.SYNC_PHASE or row[0] != 8:
            continue
        out = calc3(fn, row, rng.uniform(0.5, 40, 8))
        yield out[0], digest(*out)


OTG3_KNOWN = [  # (cp, cv, ca, tp, tv, vmax, amax, jmax): inputs of ruckig/test/test-target-known.cpp with max_jerk set
    ([0.0, -2.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, -3.0, 2.0], [0.0, 0.3, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]),
    ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]),
    ([0.0, 0.0, 0.5], [0.0, -2.2, -0.5], [0.0, 2.5, -0.5], [5.0, -2.0, -3.5], [0.0, -0.5, -2.0], [3.0, 1.0, 3.0], [3.0, 2.0, 1.0], [4.0, 3.0, 2.0]),
    ([0.2, 0.0, -0.3], [0.0, 0.2, 0.0], [0.0, 0.0, 0.1], [1.2, -0.2, 0.4], [0.0, 0.0, 0.2], [1.0, 0.5, 0.8], [2.0, 1.5, 1.0], [10.0, 8.0, 6.0]),
]


def otg3_known(fn):
    frac = np.linspace(0.05, 0.95, mog.N_SAMPLES - 2)
    pad = lambda x: np.concatenate([np.asarray(x, dtype=float), np.zeros(mog.MAXD - len(x))])
    for cp, cv, ca, tp, tv, vm, am, jm in OTG3_KNOWN:
        row = (len(cp), otg_np.SYNC_PHASE, pad(cp), pad(cv), pad(ca), pad(tp), pad(tv), pad(vm), pad(am), frac)
        out = calc3(fn, row, pad(jm))
        yield out[0], digest(*out)


def otg3_stepped_trials():
    """OTG_joints driving Ruckig::update: per trial (dof, start, vmax, amax, jmax, {tick: new goal})"""
    rng = np.random.default_rng(77)
    for trial in range(12):
        n = int(rng.integers(1, 8))
        x0 = rng.normal(0, 1, n)
        vm, am, jm = rng.uniform(0.5, 3, n), rng.uniform(1, 8, n), rng.uniform(2, 30, n)
        goals = {tick: x0 + rng.normal(0, 0.6, n) for tick in range(900) if tick % 250 == 20}  # also while still moving
        yield n, x0, vm, am, jm, goals


def otg3_stepped_ref(ref):
    """the reference's Ruckig object stepped like the wrapper does (update, pass_to_input; no more updates once the
    goal is reached until a new goal comes): one observation per update"""
    ref.rref_set_jerk.argtypes = [C.c_void_p, dp]
    for n, x0, vm, am, jm, goals in otg3_stepped_trials():
        r = ref.rref_create(n, 0.001)
        ref.rref_set_synchronization(r, otg_np.SYNC_PHASE)
        ref.rref_set_limits(r, _P(vm), _P(am))
        ref.rref_set_jerk(r, _P(jm))
        ref.rref_set_current(r, _P(x0), _P(np.zeros(n)), _P(np.zeros(n)))
        ref.rref_set_target(r, _P(x0), _P(np.zeros(n)))
        finished = False
        for tick in range(900):
            if tick in goals:
                ref.rref_set_target(r, _P(goals[tick]), _P(np.zeros(n)))
                finished = False
            if finished:
                continue
            rr = ref.rref_update(r)
            rp, rv, ra = (np.zeros(n) for _ in range(3))
            t, dur, nc = C.c_double(), C.c_double(), C.c_int()
            ref.rref_get_output(r, _P(rp), _P(rv), _P(ra), C.byref(t), C.byref(dur), C.byref(nc))
            yield rr, digest(rr, rp, rv, ra)
            if rr == 0:
                ref.rref_pass_to_input(C.c_void_p(r))
            else:
                finished = True
        ref.rref_destroy(r)


def core_calc(fn):
    """acceleration-limited one-shot calculations, phase-synchronised rows"""
    for row in mog.random_calc_inputs(4000, seed=321):
        if row[1] != otg_np.SYNC_PHASE:
            continue
        out = mog.calc_with(fn, row)
        yield out[0], digest(*out)


def core_calc8(fn):
    """core_calc for the 8-DoF generators of the 8-joint build: the rows with n = 8"""
    for row in mog.random_calc_inputs(16000, seed=3218, nmax=8, maxd=8):
        if row[1] != otg_np.SYNC_PHASE or row[0] != 8:
            continue
        out = mog.calc_with(fn, row)
        yield out[0], digest(*out)


def oracle_calc(fn):
    """acceleration-limited one-shot calculations, every row"""
    for row in mog.random_calc_inputs(3000, seed=99):
        out = mog.calc_with(fn, row)
        yield out[0], digest(*out)


def oracle_stepped(lib, pre, create):
    """Ruckig::update stepped with re-targeting through the entry points named pre + set_..., update, get_output,
    pass_to_input of one library; create(n, dt) -> handle"""
    rng = np.random.default_rng(5)
    for n in (1, 3, 6, 7):
        h = C.c_void_p(create(n, 0.004))
        getattr(lib, pre + "set_synchronization")(h, otg_np.SYNC_PHASE)
        vm, am = rng.uniform(0.5, 2, n), rng.uniform(1, 6, n)
        cur = [rng.normal(0, 1, n), np.zeros(n), np.zeros(n)]
        getattr(lib, pre + "set_limits")(h, _P(vm), _P(am))
        getattr(lib, pre + "set_current")(h, *[_P(x) for x in cur])
        for k in range(700):
            if k % 170 == 0:
                tp, tv = rng.normal(0, 1, n), (rng.normal(0, 0.2, n) if k == 340 else np.zeros(n))
                getattr(lib, pre + "set_target")(h, _P(tp), _P(tv))
            fn = getattr(lib, pre + "update")
            fn.restype = C.c_int
            r = fn(h)
            p, v, a = np.zeros(n), np.zeros(n), np.zeros(n)
            t, d, nc = C.c_double(), C.c_double(), C.c_int()
            getattr(lib, pre + "get_output")(h, _P(p), _P(v), _P(a), C.byref(t), C.byref(d), C.byref(nc))
            getattr(lib, pre + "pass_to_input")(h)
            yield r, digest(r, t.value, d.value, nc.value, p, v, a)
        getattr(lib, pre + "destroy")(h)


def _digests(seq):
    return np.array([d for _, d in seq], dtype=np.uint8)


def main():
    """record every sequence; with --append only the ones the fixture lacks, added as new members of the archive (the
    recorded ones stay as they are, byte for byte)"""
    if not otg_np.ref_available():
        raise SystemExit("oracle/_ref/libruckig_ref.so missing: run `make -C oracle ref` first")
    ref = otg_np.load_ref()
    seqs = {
        "otg3_random": lambda: otg3_random(ref.rref_calculate_and_sample_jerk),
        "otg3_known": lambda: otg3_known(ref.rref_calculate_and_sample_jerk),
        "otg3_stepped": lambda: otg3_stepped_ref(ref),
        "core_calc": lambda: core_calc(ref.rref_calculate_and_sample),
        "oracle_calc": lambda: oracle_calc(ref.rref_calculate_and_sample),
        "oracle_stepped": lambda: oracle_stepped(ref, "rref_", ref.rref_create),
        "otg3_random8": lambda: otg3_random8(ref.rref_calculate_and_sample_jerk),
        "core_calc8": lambda: core_calc8(ref.rref_calculate_and_sample),
    }
    if "--append" in sys.argv[1:]:
        import io
        import zipfile

        with np.load(FIXTURE) as z:
            have = set(z.files)
        out = {k: _digests(f()) for k, f in seqs.items() if k not in have}
        with zipfile.ZipFile(FIXTURE, "a", compression=zipfile.ZIP_DEFLATED) as zf:
            for k, v in out.items():
                buf = io.BytesIO()
                np.lib.format.write_array(buf, v, allow_pickle=False)
                zf.writestr(k + ".npy", buf.getvalue())
    else:
        out = {k: _digests(f()) for k, f in seqs.items()}
        np.savez_compressed(FIXTURE, **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()

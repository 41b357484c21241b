"""sai2b_randomize_robots (include/sai2b.h "environment sampler") on the GPU against tests/env_sampler_reference.py.

Tolerances: the counters, the counts, every affine and product row and both integer draws are exact. What goes through exp / log
(the log-uniform stiffness scale and the stiffness row), sin / cos / sqrt of the device's maths library (the tilt axis, the tilted
normal, the push directions) agrees within 4e-15 relative (floor 1 for components of unit vectors), the bound of
tests/test_env_sampler.py; the push rows, a magnitude times such a direction, within twice that plus a rounding."""
import copy

import numpy as np
import pytest

import contact_cases as cc
import env_sampler_reference as er
import plumbing
import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import _abi, sharding

pytestmark = pytest.mark.gpu

REL = 4e-15
ROBOTS = {"planar_4r": 4, "six_r": 6, "panda": 7, "sliding_base": 8}
FRAME_POS = (0.01, 0.02, 0.06)
MAX_DELAY, HW_SEED = 4, 77
ALL = ("payload", "contact", "joint_dynamics", "hardware", "push")
CFG = dict(seed=20261021, groups=ALL, payload_target="both", payload_mass_scale=(0.5, 1.5), payload_com_half=(0.01, 0.02, 0.0),
           contact_height=(-0.01, 0.03), contact_tilt_max=0.3, contact_stiffness_scale=(0.5, 2.0, 1), contact_damping_scale=(0.8, 1.2),
           contact_friction_scale=(0.5, 1.5), armature_scale=(0.5, 1.5), damping_scale=(0.0, 2.0), friction_scale=(0.9, 1.1),
           torque_limit_scale=(0.7, 1.0), delay_lower=1, delay_upper=3, lag_scale=(0.8, 1.6), gain_scale=(0.95, 1.05),
           torque_noise_scale=(0.5, 1.5), sensor_bias_half=(0.1, 0.1, 0.1, 0.01, 0.01, 0.0), sensor_noise_scale=(0.5, 2.0),
           push_force=(1.0, 10.0), push_moment=(0.0, 1.0), push_steps_lower=0, push_steps_upper=20)


def _ref_cfg(kw):
    kw = dict(kw)
    g = kw.pop("groups", ())
    kw["groups"] = g if isinstance(g, int) else sum(_abi.ENV_GROUPS[x] for x in ([g] if isinstance(g, str) else g))
    t = kw.pop("payload_target", "plant")
    kw["payload_target"] = _abi.PAYLOAD_TARGETS[t] if isinstance(t, str) else t
    for k in ("payload_com_half", "sensor_bias_half"):
        if k in kw:
            kw[k] = tuple(np.broadcast_to(np.asarray(kw[k], dtype=np.float64), (3 if k == "payload_com_half" else 6,)))
    return er.default_config(**kw)


def _mask(B, seed, p=0.5):
    return np.random.default_rng([B, seed]).uniform(size=B) < p


def _tasks(robot, hierarchy):
    n = ROBOTS[robot]
    kw = {} if robot == "panda" else dict(robot_dof=n)
    mft = pkg.motion_force_task_config("m", link=n - 1, frame_pos=FRAME_POS, **kw) if robot != "panda" else pkg.motion_force_task_config("m")
    if hierarchy == "c4":
        sel = np.zeros((2, n))
        sel[0, 0] = sel[1, n - 1] = 1
        return [mft, pkg.joint_task_config("p", sel, **kw), pkg.joint_task_config("j", **kw)]
    return [mft, pkg.joint_task_config("j", **kw)]


def _nominal(robot, B, seed, wrench_steps=None, delay=None):
    """per-robot, non-uniform rows of the five features for the whole batch"""
    n = ROBOTS[robot]
    rng = np.random.default_rng([n, B, seed])
    case = cc.draw(robot, B, 1, seed=seed)
    nom = dict(contact=case["rows"], q=case["q"], dq=0.1 * case["dq"])
    diag, off = rng.uniform(1e-3, 1e-2, (3, B)), rng.uniform(-1e-4, 1e-4, (3, B))
    nom["plant_payload"] = np.concatenate([rng.uniform(0.2, 2.0, (1, B)), rng.uniform(-0.05, 0.05, (3, B)), diag, off])
    nom["payload"] = nom["plant_payload"].copy()
    limit = rng.uniform(20, 80, (n, B))
    limit[rng.uniform(size=(n, B)) < 0.2] = np.inf
    nom["joint"] = np.concatenate([rng.uniform(0, 0.1, (n, B)), rng.uniform(0, 1, (n, B)), rng.uniform(0, 0.5, (n, B)), limit,
                                   np.full((n, B), -np.inf), np.full((n, B), np.inf)])
    d = rng.integers(0, MAX_DELAY + 1, (1, B)).astype(np.float64) if delay is None else np.full((1, B), float(delay))
    nom["actuator"] = np.concatenate([d, rng.uniform(0.3, 1.0, (n, B)), rng.uniform(0.9, 1.1, (n, B)), rng.uniform(0, 0.2, (n, B))])
    nom["sensor"] = np.concatenate([rng.uniform(-0.5, 0.5, (6, B)), rng.uniform(0, 0.1, (6, B)), rng.uniform(0.5, 1.0, (1, B))])
    steps = rng.integers(0, 3, (1, B)).astype(np.float64) if wrench_steps is None else np.full((1, B), float(wrench_steps))
    nom["wrench"] = np.concatenate([rng.normal(0, 2, (6, B)), steps]) if wrench_steps is None else np.concatenate([np.zeros((6, B)), steps])
    return nom


def _apply(g, robot, nom, cols=slice(None), payload_target="both"):
    """the five host setters with the rows of `nom` (columns `cols` of the whole batch)"""
    n = ROBOTS[robot]
    c = lambda a: np.ascontiguousarray(a[..., cols])
    p = nom["plant_payload"]
    g.set_link_payload(n - 1, c(p[0]), c(p[1:4]), c(p[4:10]), target="plant")
    if payload_target == "both":
        p = nom["payload"]
        g.set_link_payload(n - 1, c(p[0]), c(p[1:4]), c(p[4:10]), target="controller")
    r = nom["contact"]
    g.set_contact(n - 1, cc.points(1), c(r[0:3]), c(r[3:6]), c(r[6]), c(r[7]), c(r[8]), sensor_task=0)
    j = nom["joint"]
    g.set_joint_dynamics(armature=c(j[0:n]), damping=c(j[n : 2 * n]), friction=c(j[2 * n : 3 * n]), torque_limit=c(j[3 * n : 4 * n]))
    g.set_hardware(c(nom["actuator"]), c(nom["sensor"]), max_delay=MAX_DELAY, sensor_task=0, seed=HW_SEED,
                   first_robot=0 if cols == slice(None) else cols.start)
    w = nom["wrench"]
    g.set_external_wrench(n - 1, c(w[0:3]), c(w[3:6]), c(w[6]))


def _controller(robot, B, hierarchy="c3"):
    model = pkg.panda_model() if robot == "panda" else cc.model(robot)
    return pkg.Controller(model, _tasks(robot, hierarchy), B)


def _setup(robot, B, seed, cfg=None, hierarchy="c3", **nominal_kw):
    """-> (controller with the five features set, and the sampler when cfg is given; the nominal rows)"""
    nom = _nominal(robot, B, seed, **nominal_kw)
    g = _controller(robot, B, hierarchy)
    _apply(g, robot, nom)
    if cfg is not None:
        g.set_env_sampler(**cfg)
    return g, nom


def _rows(g):
    """the rows of the five features as the device holds them"""
    out = {}
    for name, target in (("payload", "controller"), ("plant_payload", "plant")):
        link, m, c, i = g.get_link_payload(target)
        if link >= 0:
            out[name] = np.concatenate([m[None], c, i])
    out["contact"] = g.get_contact()[1]
    out["joint"] = g.get_joint_dynamics()[1].reshape(-1, g.B)
    _, out["actuator"], out["sensor"] = g.get_hardware()
    out["wrench"] = g.get_external_wrench()[1]
    return out


def _reference(robot, B, cfg, nom, first_robot=0):
    c = _ref_cfg(dict(cfg, first_robot=first_robot))
    keys = ("plant_payload", "payload", "contact", "joint", "actuator", "sensor", "wrench")
    return er.EnvSamplerReference(ROBOTS[robot], B, c, {k: nom[k] for k in keys})


def _close(a, b, rel=REL, floor=1e-300):
    with np.errstate(invalid="ignore"):
        return ((a == b) | (np.abs(a - b) <= rel * np.maximum(np.abs(b), floor))).all()


def _check(g, ref, counts=None, loose_stiffness=True):
    """sample rows, counters, counts and every feature row against the restatement"""
    st, rows = g.env_sampler_state(), _rows(g)
    assert np.array_equal(st["counter"], ref.counter)
    if counts is not None:
        assert tuple(g.env_sampler_counts().values()) == counts
    loose = np.zeros(ref.total, dtype=bool)  # sample rows that go through the device's exp / sin / cos / sqrt
    unit = np.zeros(ref.total, dtype=bool)   # ... components of unit vectors among them
    if er.CONTACT in ref.first:
        f = ref.first[er.CONTACT][0]
        unit[f + 2 : f + 5] = True
        loose[f + 5] = loose_stiffness
    if er.PUSH in ref.first:
        f = ref.first[er.PUSH][0]
        unit[f + 1 : f + 4] = unit[f + 6 : f + 9] = True
    exact = ~(loose | unit)
    assert np.array_equal(st["sample"][exact], ref.sample[exact])
    assert _close(st["sample"][loose], ref.sample[loose]) and _close(st["sample"][unit], ref.sample[unit], floor=1.0)
    assert np.array_equal(plumbing.device_rows(g, _abi.BUF_ENV_SAMPLE, -1, ref.total), st["sample"])
    for name in ("plant_payload", "payload", "joint", "actuator", "sensor"):
        assert np.array_equal(rows[name], ref.rows[name]), name
    c, w = rows["contact"], ref.rows["contact"]
    assert np.array_equal(c[[0, 1, 2, 7, 8]], w[[0, 1, 2, 7, 8]]) and _close(c[3:6], w[3:6], floor=1.0)
    assert _close(c[6], w[6]) if loose_stiffness else np.array_equal(c[6], w[6])
    x, y = rows["wrench"], ref.rows["wrench"]
    assert np.array_equal(x[6], y[6])
    if er.PUSH in ref.first:
        f = ref.first[er.PUSH][0]
        mag = np.abs(ref.sample[[f, f, f, f + 5, f + 5, f + 5]])
        assert (np.abs(x[0:6] - y[0:6]) <= (2 * REL + 2.3e-16) * mag).all()
    else:
        assert np.array_equal(x, y)
    return st, rows


def _equal_columns(a, b, cols, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k][..., cols], b[k][..., cols]), (what, k)


# ------------------------------------------------------------------------------- exactness
def test_exactness_4099_pandas_every_group():
    B = 4099
    g, nom = _setup("panda", B, 1, CFG)
    twin, _ = _setup("panda", B, 1, CFG)
    ref = _reference("panda", B, CFG, nom)
    assert g.env_sampler_layout(g.get_env_sampler()) == {"payload": (0, 4), "contact": (4, 8), "joint_dynamics": (12, 28), "hardware": (40, 29),
                                                         "push": (69, 9), "total": 78}
    _check(g, ref, (0, 0))  # nothing drawn yet: zero sample rows, the nominal rows
    before = _rows(twin)
    for call in range(2):
        mask = _mask(B, 10 + call)
        counts = ref.randomize(mask)
        g.randomize_robots(mask)
        st, rows = _check(g, ref, counts)
        assert counts[0] == int(mask.sum()) and 0 < counts[1] < counts[0]
        # the controller's payload is the plant's (equal nominals, the same draw)
        assert np.array_equal(rows["payload"], rows["plant_payload"])
        if call == 0:
            _equal_columns(rows, before, ~mask, "unselected")
            assert not st["sample"][:, ~mask].any() and not st["counter"][~mask].any()
            first = {k: v.copy() for k, v in rows.items()}
            mask0 = mask
    # draws do not compound and differ from call to call
    both, only0 = mask0 & mask, mask0 & ~mask
    assert not np.array_equal(rows["contact"][:, both], first["contact"][:, both])
    _equal_columns(rows, first, only0, "not selected by the second call")
    _equal_columns(_rows(twin), before, np.ones(B, dtype=bool), "the twin never made the call")
    s = st["sample"]
    drawn = mask0 | mask
    assert ((s[0, drawn] >= 0.5) & (s[0, drawn] <= 1.5)).all() and ((s[9, drawn] >= 0.5 * (1 - 1e-14)) & (s[9, drawn] <= 2.0 * (1 + 1e-14))).all()
    assert set(np.unique(s[40, drawn])) == {1.0, 2.0, 3.0} and (rows["actuator"][1:8] <= 1.0).all()


# ------------------------------------------------------------------------------- sizes and edges
GROUP_SETS = [("payload",), ("contact",), ("joint_dynamics",), ("hardware",), ("push",), ALL]


@pytest.mark.parametrize("robot", list(ROBOTS))
def test_sizes_and_edges(robot):
    import torch

    for B in (1, 63, 64, 65, 200):
        g, nom = _setup(robot, B, 2, CFG)
        ref = _reference(robot, B, CFG, nom)
        n = ROBOTS[robot]
        assert ref.total == 29 + 7 * n == g.env_sampler_layout(g.get_env_sampler())["total"]
        # an empty mask writes nothing
        g.randomize_robots(np.zeros(B, dtype=bool))
        _check(g, ref, (0, 0))
        for k, groups in enumerate(GROUP_SETS):
            mask = _mask(B, 20 + k) if B > 1 else np.array([True])
            bits = sum(_abi.ENV_GROUPS[x] for x in groups)
            counts = ref.randomize(mask, bits)
            if k % 2:  # a device mask gives what a host mask gives
                g.randomize_robots(torch.from_numpy(mask).cuda(), groups)
            else:
                g.randomize_robots(mask, groups if k else bits)
            _check(g, ref, counts)
        g.close()


# ------------------------------------------------------------------------------- consumed like a setter's rows
@pytest.mark.parametrize("hierarchy", ["c3", "c4"])
def test_drawn_rows_are_consumed_like_a_setters(hierarchy):
    B = 200
    g, nom = _setup("panda", B, 4, CFG, hierarchy)
    g.randomize_robots(np.ones(B, dtype=bool))
    rows = _rows(g)
    assert (rows["actuator"][15:22] > 0).any() and (rows["sensor"][6:12] > 0).any()  # actuator and sensor noise are on
    twin = _controller("panda", B, hierarchy)
    _apply(twin, "panda", rows)
    runs = []
    for c in (g, twin):
        c.set_state(nom["q"], nom["dq"])
        c.reinitialize()
        out = []
        for _ in range(6):
            tau = c.tick()
            c.sim_step(None, substeps=2)
            out.append((tau,) + c.get_state() + (plumbing.device_rows(c, _abi.BUF_SENSED, 0, 6), plumbing.device_rows(c, _abi.BUF_TAU_APPLIED, -1, 7)))
        runs.append(out)
    for period, (a, b) in enumerate(zip(*runs)):
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y, equal_nan=True), (period, k)
    assert g.get_external_wrench_state()["robots_pushed"] > 0 and np.abs(runs[0][-1][3]).max() > 0  # pushes and contact took place


# ------------------------------------------------------------------------------- no compounding
def test_unit_ranges_keep_the_nominal_and_a_new_set_follows_the_setters():
    B = 130
    unit = dict(seed=5, groups=ALL, payload_target="both", delay_lower=2, delay_upper=2)
    g, nom = _setup("sliding_base", B, 5, unit, wrench_steps=0, delay=2)
    before = _rows(g)
    for k in range(5):
        g.randomize_robots(_mask(B, 40 + k, 0.7))
    _equal_columns(_rows(g), before, np.ones(B, dtype=bool), "unit ranges")
    assert np.array_equal(g.env_sampler_state()["counter"], sum(_mask(B, 40 + k, 0.7).astype(int) for k in range(5)))
    # non-trivial ranges: five calls on one robot give five draws of the same nominal, never a product of draws
    cfg = dict(CFG, seed=6)
    g.set_env_sampler(**cfg)
    ref = _reference("sliding_base", B, cfg, nom)
    ones = np.ones(B, dtype=bool)
    for k in range(5):
        counts = ref.randomize(ones)
        g.randomize_robots(ones)
    _check(g, ref, counts)
    # new planes through the setter: the nominal is still the old one until the sampler is set again
    new = cc.draw("sliding_base", B, 1, seed=9)["rows"]
    g.set_contact(7, cc.points(1), new[0:3], new[3:6], new[6], new[7], new[8], sensor_task=0)
    counts = ref.randomize(ones, er.CONTACT)
    g.randomize_robots(ones, "contact")
    _check(g, ref, counts)  # (drawn from the OLD nominal: the header says so)
    g.set_contact(7, cc.points(1), new[0:3], new[3:6], new[6], new[7], new[8], sensor_task=0)
    g.set_env_sampler(**cfg)
    ref2 = _reference("sliding_base", B, cfg, dict(_rows(g)))
    assert np.array_equal(ref2.nominal["contact"], new) and not g.env_sampler_state()["counter"].any()
    counts = ref2.randomize(ones, er.CONTACT)
    g.randomize_robots(ones, "contact")
    _check(g, ref2, counts)


# ------------------------------------------------------------------------------- clearance interplay
def test_reset_clearance_sees_the_drawn_plane():
    import test_gpu_reset_sampler as tg

    contact, env, new, mask = er.clearance_case()  # (tests/test_env_sampler.py holds its candidates away from the threshold)
    B = new.shape[1]
    g, ref, m = tg._generic("panda", B, er.CLEARANCE_SEED, dict(goal_tasks=(0, 1), **er.CLEARANCE_RESET), contact=contact)
    old = copy.copy(ref)
    old.margins = []
    g.set_env_sampler(groups=("contact",), **env)
    g.randomize_robots(np.ones(B, dtype=bool))
    got = g.get_contact()[1]
    assert np.array_equal(got[[0, 1, 2, 7, 8]], new[[0, 1, 2, 7, 8]]) and _close(got[3:6], new[3:6], floor=1.0) and _close(got[6], new[6])
    ref.contact = new
    out, out_old = ref.reset(mask), old.reset(mask)
    assert ref.borderline() == 0  # no candidate within 1e-9 m of the threshold
    assert not np.array_equal(out["tries"], out_old["tries"])  # the new plane changes who is accepted
    g.reset_robots_sampled(mask)
    tg._check_draws(g, ref, out, mask, ["mft", "jt"])
    # every accepted start clears the NEW plane, on the oracle's pose
    q = g.get_state()[0]
    accepted = mask & ~out["exhausted"]
    pts = ref.kin(np.where(accepted, q, 0.0))["points"]
    d = np.einsum("ib,kib->kb", new[3:6], new[0:3][None] - pts)
    assert accepted.any() and (d[:, accepted] <= -0.01).all()


# ------------------------------------------------------------------------------- push only, mid-episode
def test_push_only_on_a_sparse_mask_mid_episode():
    B = 640
    cfg = dict(CFG, push_steps_lower=3, push_steps_upper=5)
    g, nom = _setup("panda", B, 7, cfg, wrench_steps=0)
    ref = _reference("panda", B, cfg, nom)
    g.set_state(nom["q"], nom["dq"])
    g.reinitialize()
    for _ in range(3):
        g.tick(want_output=False)
        g.sim_step(None)
    assert g.get_external_wrench_state()["robots_pushed"] == 0
    mask = np.zeros(B, dtype=bool)
    mask[[3, 64, 127, 128, 401, 639]] = True  # 1 %
    before = _rows(g)
    counts = ref.randomize(mask, er.PUSH)
    g.randomize_robots(mask, "push")
    st, rows = _check(g, ref, counts)
    assert counts == (6, 0) and np.array_equal(st["counter"], mask.astype(int))
    for k in before:
        if k != "wrench":
            assert np.array_equal(rows[k], before[k]), k  # other groups' rows: untouched bit for bit
    assert not st["sample"][:69].any() and not st["sample"][69:, ~mask].any()
    steps = rows["wrench"][6]
    assert ((steps[mask] >= 3) & (steps[mask] <= 5)).all() and not steps[~mask].any()
    for k in range(1, 7):
        g.tick(want_output=False)
        g.sim_step(None)
        assert g.get_external_wrench_state()["robots_pushed"] == int((steps - (k - 1) > 0).sum())  # == the mask's count at k = 1
        assert np.array_equal(g.get_external_wrench()[1][6], np.maximum(steps - k, 0))


# ------------------------------------------------------------------------------- reproducibility
def test_two_shards_equal_one_context():
    B, robot = 4099, "panda"
    g, nom = _setup(robot, B, 8, CFG)
    masks = [_mask(B, 60), _mask(B, 61, 0.3)]
    for m in masks:
        g.randomize_robots(m)
    one, st = _rows(g), g.env_sampler_state()
    for rank in range(2):
        lo, hi = sharding.shard_bounds(B, 2, rank)
        s = _controller(robot, hi - lo)
        _apply(s, robot, nom, slice(lo, hi))
        sharding.set_env_sampler(s, 2, rank, B, **CFG)
        assert s.get_env_sampler().first_robot == lo
        for m in masks:
            sharding.randomize_robots(s, 2, rank, m)
        part, ps = _rows(s), s.env_sampler_state()
        for k in one:
            assert np.array_equal(part[k], one[k][..., lo:hi]), k
        assert np.array_equal(ps["sample"], st["sample"][:, lo:hi]) and np.array_equal(ps["counter"], st["counter"][lo:hi])
        s.close()


def _state(g):
    st = g.env_sampler_state()
    return dict(_rows(g), sample=st["sample"], counter=st["counter"])


def test_snapshot_banks_hold_the_counter_and_the_sample_rows():
    B = 200
    what = _abi.SNAP_EPISODE | _abi.SNAP_ENVIRONMENT
    h, nom = _setup("panda", B, 9, CFG)
    blocks = {r["block"]: r for r in h.snapshot_layout(what)}
    assert blocks["env_sampler_counter"]["rows"] == 1 and blocks["env_sampler_counter"]["elem_bytes"] == 4
    assert blocks["env_sampler_sample"]["rows"] == 78 and blocks["env_sampler_sample"]["elem_bytes"] == 8
    assert "env_sampler_sample" not in {r["block"] for r in h.snapshot_layout(_abi.SNAP_EPISODE)}
    assert "env_sampler_counter" not in {r["block"] for r in h.snapshot_layout(_abi.SNAP_ENVIRONMENT)}
    mask, ones = _mask(B, 70), np.ones(B, dtype=bool)
    bank = h.snapshot_bank(B, what)
    start = _state(h)
    bank.save()
    h.randomize_robots(mask)
    first = _state(h)
    assert not np.array_equal(first["contact"][:, mask], start["contact"][:, mask])
    bank.load()
    _equal_columns(_state(h), start, ones, "after load")  # counter, sample rows and environment rows, bit for bit
    h.randomize_robots(mask)
    _equal_columns(_state(h), first, ones, "the same draw again")
    # export and import into a fresh context: the sequence continues with the second draw
    bank.save()
    f, _ = _setup("panda", B, 9, CFG)
    fb = f.snapshot_bank(B, what)
    fb.import_(bank.export())
    fb.load()
    _equal_columns(_state(f), first, ones, "imported")
    for c in (h, f):
        c.randomize_robots(ones)
    second = _state(h)
    _equal_columns(_state(f), second, ones, "second draw after import")
    assert not np.array_equal(second["contact"][:, mask], first["contact"][:, mask])
    # one slot cloned into every robot: identical plants, the sample rows that describe them, one counter
    fb.save()
    fb.load(slots=np.full(B, 5, dtype=np.int32))
    clone = _state(f)
    for k, v in clone.items():
        assert np.array_equal(v, np.broadcast_to(second[k][..., 5:6], v.shape)), k
    # a bank made before the sampler was configured does not fit afterwards
    p, _ = _setup("panda", B, 9)
    pb = p.snapshot_bank(B, what)
    p.set_env_sampler(**CFG)
    with pytest.raises(ValueError, match="env_sampler"):
        pb.save()
    for b_ in (bank, fb, pb):
        b_.close()


# ------------------------------------------------------------------------------- argument checks
def test_argument_checks():
    B = 5
    ones = np.ones(B, dtype=bool)
    g = _controller("panda", B)
    with pytest.raises(ValueError, match="no environment sampler is configured"):
        g.randomize_robots(ones)
    for call in (g.env_sampler_counts, g.env_sampler_state, g.get_env_sampler):
        with pytest.raises(ValueError, match="no environment sampler is configured"):
            call()
    assert not g.device_buffer(_abi.BUF_ENV_SAMPLE)
    # a group whose feature is not in force: each has its message, and the context stays without a sampler
    needs = dict(payload="needs a plant payload", contact="needs a contact", joint_dynamics="needs joint dynamics", hardware="needs hardware",
                 push="needs an external wrench")
    for name, msg in needs.items():
        with pytest.raises(ValueError, match=msg):
            g.set_env_sampler(groups=(name,))
    nom = _nominal("panda", B, 11)
    p = nom["plant_payload"]
    g.set_link_payload(6, p[0], p[1:4], p[4:10], target="plant")
    with pytest.raises(ValueError, match="needs a controller payload on the plant payload's link"):
        g.set_env_sampler(groups=("payload",), payload_target="both")
    g.set_link_payload(5, p[0], p[1:4], p[4:10], target="controller")
    with pytest.raises(ValueError, match="needs a controller payload on the plant payload's link"):
        g.set_env_sampler(groups=("payload",), payload_target="both")
    with pytest.raises(ValueError, match="no environment sampler is configured"):
        g.randomize_robots(ones)
    _apply(g, "panda", nom)
    with pytest.raises(ValueError, match="delay_upper exceeds max_delay of the hardware in force"):
        g.set_env_sampler(**dict(CFG, delay_upper=MAX_DELAY + 1))
    with pytest.raises(ValueError, match="lag_scale: lower must be > 0"):
        g.set_env_sampler(**dict(CFG, lag_scale=(0.0, 1.0)))
    g.set_env_sampler(**CFG)
    before = _state(g)
    assert g.lib.sai2b_randomize_robots(g.h, None, 0, 0) == _abi.INVALID_ARGUMENT and b"mask is NULL" in g.lib.sai2b_last_error(g.h)
    with pytest.raises(ValueError, match="a mask of one entry per robot"):
        g.randomize_robots(None)
    assert g.lib.sai2b_randomize_robots(g.h, ones.view(np.uint8).ctypes.data, 32, 0) == _abi.INVALID_ARGUMENT
    # a feature cleared since: the groups that need it are refused, the others still run
    g.clear_contact()
    for groups in (0, "contact"):
        with pytest.raises(ValueError, match="SAI2B_ENV_CONTACT needs a contact"):
            g.randomize_robots(ones, groups)
    # a hardware set since with a shallower history
    g.set_hardware(max_delay=2)
    with pytest.raises(ValueError, match="delay_upper exceeds max_delay"):
        g.randomize_robots(ones, "hardware")
    after = _state(g)
    for k in ("plant_payload", "payload", "joint", "wrench", "sample", "counter"):
        assert np.array_equal(after[k], before[k]), k  # nothing was launched
    assert tuple(g.env_sampler_counts().values()) == (0, 0)
    g.randomize_robots(ones, ("payload", "push"))
    assert tuple(g.env_sampler_counts().values()) == (B, 0) and (g.env_sampler_state()["counter"] == 1).all()
    assert g.get_env_sampler().seed == CFG["seed"]
    g.clear_env_sampler()
    with pytest.raises(ValueError, match="no environment sampler is configured"):
        g.randomize_robots(ones)
    assert not g.device_buffer(_abi.BUF_ENV_SAMPLE)


# ------------------------------------------------------------------------------- the resident loop
def test_resident_loop_device_mask_equals_numpy_mask():
    import torch

    B = 200
    runs = []
    for device in (True, False):
        g, nom = _setup("panda", B, 12, CFG)
        g.set_reset_sampler(seed=3, goal_tasks=(0, 1), max_tries=4, clearance=0.0)
        g.set_observation(blocks=("q",), max_episode_steps=5, max_joint_speed=0.9)  # (the speed limit spreads the ends over the periods)
        ones = np.ones(B, dtype=bool)
        g.randomize_robots(ones)
        g.reset_robots_sampled(ones)
        done = torch.zeros(B, dtype=torch.uint8, device="cuda") if device else None
        out = torch.zeros((g.observation_rows(), B), dtype=torch.float64, device="cuda") if device else None
        trace = []
        for _ in range(20):
            g.tick(want_output=False)
            g.sim_step(None)
            if device:
                g.observe(out, done)
                g.randomize_robots(done)  # ahead of the reset: its clearance criterion sees the new plane
                g.reset_robots_sampled(done)
                d = done.cpu().numpy() != 0
            else:
                _, d8 = g.observe()
                g.randomize_robots(d8)
                g.reset_robots_sampled(d8)
                d = d8 != 0
            trace.append((d, g.get_state()[0], g.reset_sampler_state()["tries"]))
        runs.append((trace, _state(g)))
    for (da, qa, ta), (db, qb, tb) in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(da, db) and np.array_equal(qa, qb, equal_nan=True) and np.array_equal(ta, tb)
    _equal_columns(runs[0][1], runs[1][1], np.ones(B, dtype=bool), "device against numpy")
    ends = [int(d.sum()) for d, _, _ in runs[0][0]]
    assert sum(ends) > B and len(set(ends)) > 3  # masks of several sizes
    assert np.array_equal(runs[0][1]["counter"], 1 + sum(d.astype(int) for d, _, _ in runs[0][0]))

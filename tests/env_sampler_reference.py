"""CPU restatement of the environment sampler's law (include/sai2b.h "environment sampler"; numpy float64, no GPU; test
infrastructure) on top of tests/hardware_reference.py's Philox. Every draw is a function of (draw counter, robot, key, the ranges,
the nominal rows) alone. A range is (lower, upper, log_uniform); numpy evaluates a * b + c as a product and a sum, never fused."""
import numpy as np

import hardware_reference as hr
import reset_sampler_reference as rr

PAYLOAD, CONTACT, JOINT, HARDWARE, PUSH = 1, 2, 4, 8, 16
GROUPS = (PAYLOAD, CONTACT, JOINT, HARDWARE, PUSH)
STREAM = {PAYLOAD: 5, CONTACT: 6, JOINT: 7, HARDWARE: 8, PUSH: 9}
RANGES = ("payload_mass_scale", "contact_height", "contact_stiffness_scale", "contact_damping_scale", "contact_friction_scale",
          "armature_scale", "damping_scale", "friction_scale", "torque_limit_scale", "lag_scale", "gain_scale", "torque_noise_scale",
          "sensor_noise_scale", "push_force", "push_moment")
JOINT_RANGES = ("armature_scale", "damping_scale", "friction_scale", "torque_limit_scale")
HW_RANGES = ("lag_scale", "gain_scale", "torque_noise_scale")


def default_config(**kw):
    """the library's defaults as a dict (ranges as (lower, upper, log_uniform)), with `kw` on top"""
    c = {name: (1.0, 1.0, 0) for name in RANGES}
    for name in ("contact_height", "push_force", "push_moment"):
        c[name] = (0.0, 0.0, 0)
    c.update(seed=0, first_robot=0, groups=0, payload_target=2, payload_com_half=(0.0, 0.0, 0.0), contact_tilt_max=0.0,
             sensor_bias_half=(0.0,) * 6, delay_lower=0, delay_upper=0, push_steps_lower=0, push_steps_upper=0)
    for k, v in kw.items():
        assert k in c, k
        c[k] = tuple(v) + (0,) * (3 - len(v)) if k in RANGES else v
    return c


def group_rows(group, dof):
    return {PAYLOAD: 4, CONTACT: 8, JOINT: 4 * dof, HARDWARE: 8 + 3 * dof, PUSH: 9}[group]


def layout(groups, dof):
    """-> ({group bit: (first row, rows)}, total) of the sample rows"""
    out, total = {}, 0
    for g in GROUPS:
        if groups & g:
            out[g] = (total, group_rows(g, dof))
            total += out[g][1]
    return out, total


def uniforms4(c, stream, call, robot, key):
    """[4][...] uniforms of one call: counter (0, c, 256 stream + call, robot), u = (x + 0.5) 2^-32; key: (k0, k1) words"""
    w = hr.philox4x32_10((np.zeros_like(np.asarray(c)), c, 256 * stream + np.asarray(call), robot), key)
    return (w.astype(np.float64) + 0.5) * 2.0**-32


def key_of(seed):
    return (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def draw_range(r, u):
    """r: (lower, upper, log_uniform), each a scalar or an array like u"""
    lo, hi, lg = (np.asarray(x, dtype=np.float64) for x in r)
    lin = lo + (hi - lo) * u
    with np.errstate(divide="ignore", invalid="ignore"):
        la, lb = np.log(lo), np.log(hi)
        e = np.exp(la + (lb - la) * u)
    return np.where(lg != 0, e, lin)


def draw_int(lo, hi, u):
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    return (lo + np.minimum(np.floor((hi - lo + 1).astype(np.float64) * u).astype(np.int64), hi - lo)).astype(np.float64)


def offset(half, u):
    return np.asarray(half, dtype=np.float64) * (2.0 * u - 1.0)


def direction(u0, u1):
    c, phi = 2.0 * u0 - 1.0, 6.283185307179586 * u1
    r = np.sqrt(1.0 - c * c)
    return np.stack([r * np.cos(phi), r * np.sin(phi), c])


def payload(cfg, c, robot, key, nominal):
    """nominal [10][...] -> (rows [10][...], sample [4][...])"""
    u = uniforms4(c, 5, 0, robot, key)
    s = draw_range(cfg["payload_mass_scale"], u[0])
    o = np.stack([offset(np.asarray(cfg["payload_com_half"])[k], u[1 + k]) for k in range(3)])
    return payload_apply(np.concatenate([s[None], o]), nominal), np.concatenate([s[None], o])


def payload_apply(sample, nominal):
    return np.concatenate([(nominal[0] * sample[0])[None], nominal[1:4] + sample[1:4], nominal[4:10] * sample[0]])


def contact(cfg, c, robot, key, nominal):
    """nominal [9][...] -> (rows [9][...], sample [8][...])"""
    u, v = uniforms4(c, 6, 0, robot, key), uniforms4(c, 6, 1, robot, key)
    h = draw_range(cfg["contact_height"], u[0])
    theta = np.asarray(cfg["contact_tilt_max"], dtype=np.float64) * u[1]
    axis, D = rr.axis_rotation(theta, u[2], u[3])
    n = nominal[3:6]
    p = nominal[0:3] + h * n
    turned = np.stack([(D[3 * k] * n[0] + D[3 * k + 1] * n[1]) + D[3 * k + 2] * n[2] for k in range(3)])
    nn = np.where(theta != 0.0, turned, n)
    names = ("contact_stiffness_scale", "contact_damping_scale", "contact_friction_scale")
    s = np.stack([draw_range(cfg[names[k]], v[k]) for k in range(3)])
    return np.concatenate([p, nn, nominal[6:9] * s]), np.concatenate([h[None], theta[None], axis, s])


def scales(r, c, stream, first_call, robot, key, count):
    """[count][...] per-joint scales: joint i takes word i mod 4 of call first_call + i / 4"""
    u = np.concatenate([uniforms4(c, stream, first_call + j, robot, key) for j in range((count + 3) // 4)])[:count]
    return draw_range(r, u)


def joint(cfg, c, robot, key, nominal, dof):
    """nominal [4 dof][...] -> (rows, sample), both [4 dof][...]"""
    s = np.concatenate([scales(cfg[JOINT_RANGES[p]], c, 7, 2 * p, robot, key, dof) for p in range(4)])
    return nominal * s, s


def hardware(cfg, c, robot, key, act, sensor, dof):
    """act [1 + 3 dof][...], sensor [12 or 13][...] nominal -> (act rows, sensor rows [12], sample [8 + 3 dof], lag clipped [...] bool)"""
    delay = draw_int(cfg["delay_lower"], cfg["delay_upper"], uniforms4(c, 8, 0, robot, key)[0])
    s = np.concatenate([scales(cfg[HW_RANGES[p]], c, 8, 1 + 2 * p, robot, key, dof) for p in range(3)])
    rows = act[1:] * s
    clipped = (rows[:dof] > 1.0).any(axis=0)
    rows[:dof] = np.minimum(rows[:dof], 1.0)
    u = np.concatenate([uniforms4(c, 8, 7, robot, key), uniforms4(c, 8, 8, robot, key)])
    half = np.asarray(cfg["sensor_bias_half"], dtype=np.float64)
    o = np.stack([offset(half[k], u[k]) for k in range(6)])
    sn = draw_range(cfg["sensor_noise_scale"], u[6])
    return (np.concatenate([delay[None], rows]), np.concatenate([sensor[0:6] + o, sensor[6:12] * sn]),
            np.concatenate([delay[None], s, o, sn[None]]), clipped)


def push(cfg, c, robot, key):
    """-> (rows [7][...], sample [9][...])"""
    u, v = uniforms4(c, 9, 0, robot, key), uniforms4(c, 9, 1, robot, key)
    f, m = draw_range(cfg["push_force"], u[0]), draw_range(cfg["push_moment"], v[0])
    df, dm = direction(u[1], u[2]), direction(v[1], v[2])
    steps = draw_int(cfg["push_steps_lower"], cfg["push_steps_upper"], u[3])
    return np.concatenate([f * df, m * dm, steps[None]]), np.concatenate([f[None], df, steps[None], m[None], dm])


class EnvSamplerReference:
    """cfg: default_config(...). nominal: dict of the feature rows at set time, for the groups of cfg: plant_payload [10][B],
    payload [10][B] (payload_target 3), contact [9][B], joint [6 dof][B], actuator [1 + 3 dof][B], sensor [13][B], wrench [7][B].
    self.rows holds the rows as the device has them after the calls so far."""

    def __init__(self, dof, B, cfg, nominal):
        self.dof, self.B, self.cfg = dof, B, dict(cfg)
        self.nominal = {k: np.array(v, dtype=np.float64) for k, v in nominal.items()}
        self.rows = {k: v.copy() for k, v in self.nominal.items()}
        self.first, self.total = layout(cfg["groups"], dof)
        self.sample = np.zeros((self.total, B))
        self.counter = np.zeros(B, dtype=np.int64)
        self.robot = cfg["first_robot"] + np.arange(B)
        self.key = key_of(cfg["seed"])

    def randomize(self, mask, groups=0):
        """-> counts (drawn, lag clipped)"""
        cfg, n = self.cfg, self.dof
        m = np.flatnonzero(np.asarray(mask))
        groups = groups or cfg["groups"]
        assert not groups & ~cfg["groups"]
        c, robot, clipped = self.counter[m], self.robot[m], 0

        def put(group, sample):
            f, rows = self.first[group]
            self.sample[f : f + rows, m] = sample

        if len(m) and groups & PAYLOAD:
            rows, s = payload(cfg, c, robot, self.key, self.nominal["plant_payload"][:, m])
            self.rows["plant_payload"][:, m] = rows
            if cfg["payload_target"] == 3:
                self.rows["payload"][:, m] = payload_apply(s, self.nominal["payload"][:, m])
            put(PAYLOAD, s)
        if len(m) and groups & CONTACT:
            rows, s = contact(cfg, c, robot, self.key, self.nominal["contact"][:, m])
            self.rows["contact"][:, m] = rows
            put(CONTACT, s)
        if len(m) and groups & JOINT:
            rows, s = joint(cfg, c, robot, self.key, self.nominal["joint"][: 4 * n, m], n)
            self.rows["joint"][: 4 * n, m] = rows
            put(JOINT, s)
        if len(m) and groups & HARDWARE:
            act, sen, s, clip = hardware(cfg, c, robot, self.key, self.nominal["actuator"][:, m], self.nominal["sensor"][:, m], n)
            self.rows["actuator"][:, m], self.rows["sensor"][:12, m] = act, sen
            clipped = int(clip.sum())
            put(HARDWARE, s)
        if len(m) and groups & PUSH:
            rows, s = push(cfg, c, robot, self.key)
            self.rows["wrench"][:, m] = rows
            put(PUSH, s)
        self.counter[m] += 1
        return len(m), clipped


# the clearance interplay of tests/test_gpu_env_sampler.py: drawn height and tilt, then the episode sampler's clearance criterion.
# Chosen so that no candidate of any try lies within 1e-9 m of the threshold on the new planes (tests/test_env_sampler.py checks it
# on the CPU).
CLEARANCE_SEED, CLEARANCE_RESET = 13, dict(max_tries=6, clearance=0.01)


def clearance_case(B=65, robot="panda"):
    """-> (contact case of contact_cases.draw, the env sampler's arguments, the planes after one draw of every robot [9][B], the
    reset's mask)"""
    import contact_cases as cc

    case = cc.draw(robot, B, 1, seed=2)
    env = dict(seed=31, contact_height=(-0.02, 0.05), contact_tilt_max=0.4)
    cfg = default_config(groups=CONTACT, **env)
    rows, _ = contact(cfg, np.zeros(B, dtype=np.int64), np.arange(B), key_of(env["seed"]), case["rows"])
    mask = np.random.default_rng([B, 50]).uniform(size=B) < 0.8
    return case, env, rows, mask

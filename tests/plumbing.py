"""Inputs for the Panda hierarchies in which every per-robot row a tick kernel reads is visible in its results
(tests/test_gpu_kernel_plumbing.py), and the read-back of the tasks' integrators on both sides.

Built on workloads.make_inputs, which stays as it is (bench.py and the golden fixtures depend on it): its q, dq and
MotionForceTask goals are already non-zero and differ per robot and row; here the JointTask goals dq and ddq, the goal
and sensed wrench, and motion of q and dq over the ticks are added. The gains add integral terms to every task (and a
closed-loop force and moment space along generic axes where the MotionForceTask is full), so that every integrator
row moves the torques. A set of robots is put into a singular pose for a tick and taken out again: at the next tick
their MotionForceTask istate row says they are leaving a region, and the SVD-free kernels must decline them.
"""
import ctypes as C

import numpy as np

import oracle_lib as ol
import sai2_primitives_perso_amd as pkg
from sai2_primitives_perso_amd import workloads as wl

N = pkg.DOF
WARMUP = 3  # ticks before the ones a test looks at: every integrator is non-zero and differs per robot by then
# generic directions: no world axis is orthogonal to either, so every goal, sensed and integrator row of the force and
# moment spaces, and of the motion spaces orthogonal to them, reaches the torques
FORCE_AXIS = (0.36, -0.48, 0.8)
MOMENT_AXIS = (-0.6, 0.64, 0.48)
ELBOW_STRETCHED = -0.0715  # q4 next to its upper limit: the arm is stretched, the 6-row task singular
MFT_KEYS = (("pos", 3), ("rot", 9), ("v", 3), ("w", 3), ("a", 3), ("alpha", 3), ("f", 3), ("m", 3), ("sf", 3), ("sm", 3))


def modified_model(model):
    """the 7-joint arm of test_gpu_parity.test_modified_robot_model_runtime_constants: not the built-in Panda, so the
    SVD-free kernel reads the model from the ctx parameter block (tick_fast_kernel<*, false>)"""
    model.joint_xyz[2][1] = -0.29
    model.joint_xyz[4][1] = 0.41
    model.joint_rpy[3][1] = 0.2
    model.link_mass[1] = 4.2
    model.link_com[5][2] = 0.03
    for k, v in enumerate((0.12, 0.08, 0.1, 0.01, -0.02, 0.015)):
        model.link_inertia[4][k] = v
    return model


def _gains(cfg, force):
    if cfg.type == pkg.MOTION_FORCE_TASK:
        for i in range(3):
            cfg.ki_pos[i], cfg.ki_ori[i] = 4.0 + i, 2.0 + 0.5 * i
        if force:
            cfg.force_space_dimension = cfg.moment_space_dimension = 1
            cfg.closed_loop_force = cfg.closed_loop_moment = 1
            cfg.passivity_enabled = 0
            for i in range(3):
                cfg.force_axis[i], cfg.moment_axis[i] = FORCE_AXIS[i], MOMENT_AXIS[i]
                cfg.ki_force[i], cfg.ki_moment[i] = 1.3 + 0.1 * i, 0.9 + 0.1 * i
    else:
        for i in range(len(cfg.ki)):
            cfg.ki[i] = 3.0 + 0.25 * i
    return cfg


def configs(tasks, force):
    """(oracle configs, product configs) of a make_inputs hierarchy with the integral gains (and force space) on"""
    return ([_gains(c, force) for c in ol.task_configs(tasks)], [_gains(c, force) for c in pkg.task_configs(tasks)])


class Inputs:
    """Per-tick inputs of a batch: `at(k)` -> {"q", "dq", "mft{t}.<key>", "jt{t}.<key>": [rows][B]}.
    singular[k]: the robots put into the stretched pose at tick k (they leave it at k + 1)."""

    def __init__(self, config, B, seed, blend=True):
        inp = wl.make_inputs(config, B=B, seed=seed)
        rng = np.random.default_rng([seed, B, 11])
        self.config, self.B, self.tasks = config, B, inp["tasks"]
        self.base = {"q": inp["q"], "dq": inp["dq"]}
        for t, (kind, _) in enumerate(self.tasks):
            g = inp[f"{kind}{t}"]
            if kind == "mft":
                for key in ("pos", "rot", "v", "w", "a", "alpha"):
                    self.base[f"mft{t}.{key}"] = g[key]
                self.base[f"mft{t}.f"] = rng.normal(0, 4.0, size=(3, B))
                self.base[f"mft{t}.m"] = rng.normal(0, 0.4, size=(3, B))
                self.base[f"mft{t}.sf"] = rng.normal(0, 4.0, size=(3, B))
                self.base[f"mft{t}.sm"] = rng.normal(0, 0.4, size=(3, B))
            else:
                k0 = g["q"].shape[0]
                self.base[f"jt{t}.q"] = g["q"]
                self.base[f"jt{t}.dq"] = rng.normal(0, 0.2, size=(k0, B))
                self.base[f"jt{t}.ddq"] = rng.normal(0, 0.5, size=(k0, B))
        self.amp = rng.uniform(0.002, 0.01, size=(N, B))
        self.phase = rng.uniform(0, 2 * np.pi, size=(2, N, B))
        self.singular = {}
        if blend:
            # every 23rd robot from the last one on (so the last, partial wavefront has one), in two groups: singular at
            # the last warm-up tick and again two ticks later, or once later still
            robots = np.arange(B - 1, -1, -23)
            for k in (WARMUP - 1, WARMUP + 2):
                self.singular[k] = robots[0::2]
            self.singular[WARMUP + 3] = robots[1::2]
        if config == 4:
            # the stretched elbow leaves the 3-row position task regular for most poses: Panda poses with it whose
            # position Jacobian has s_2 / s_0 well inside the blending region (s_min = 0.006, s_max = 0.06)
            q = wl.sample_poses(rng, 4096)
            q[:, 3] = ELBOW_STRETCHED
            s = np.linalg.svd(wl.frame_jacobian(*wl.fk(q))[0][:, :3], compute_uv=False)
            self.pool = np.ascontiguousarray(q[(s[:, 2] > 0.012 * s[:, 0]) & (s[:, 2] < 0.04 * s[:, 0])].T)
            assert self.pool.shape[1] >= 16
        self.extra = []  # (key, row, robot, delta, ticks) added on top: tests perturb single entries

    def at(self, k):
        x = {key: a.copy() for key, a in self.base.items()}
        x["q"] = x["q"] + self.amp * np.sin(0.9 * k + self.phase[0])
        x["dq"] = x["dq"] * (1.0 + 0.3 * np.sin(0.6 * k + self.phase[1]))
        if k in self.singular:
            r = self.singular[k]
            if self.config == 4:  # the position task: a pose of the pool, one per robot
                x["q"][:, r] = self.pool[:, r % self.pool.shape[1]]
            else:
                x["q"][3, r] = ELBOW_STRETCHED
        for key, row, robot, delta, ticks in self.extra:
            if k in ticks:
                x[key][row, robot] += delta
        return x

    def select(self, idx):
        """the same robots in another order or a subset of them, as a batch of their own"""
        out = object.__new__(Inputs)
        out.config, out.B, out.tasks = self.config, len(idx), self.tasks
        out.base = {key: np.ascontiguousarray(a[:, idx]) for key, a in self.base.items()}
        out.amp, out.phase = self.amp[:, idx], self.phase[..., idx]
        if self.config == 4:
            out.pool = self.pool[:, np.arange(self.B)[idx] % self.pool.shape[1]]
        where = np.full(self.B, -1)
        where[idx] = np.arange(len(idx))
        out.singular = {k: where[r][where[r] >= 0] for k, r in self.singular.items()}
        out.extra = []
        return out


def feed(ctrl, tasks, x):
    """one tick's inputs into an Oracle or a pkg.Controller"""
    ctrl.set_state(x["q"], x["dq"])
    for t, (kind, _) in enumerate(tasks):
        if kind == "mft":
            ctrl.set_mft_goals(t, *(x[f"mft{t}.{k}"] for k in ("pos", "rot", "v", "w", "a", "alpha")))
            ctrl.set_mft_goal_wrench(t, x[f"mft{t}.f"], x[f"mft{t}.m"])
            ctrl.set_mft_sensed_wrench(t, x[f"mft{t}.sf"], x[f"mft{t}.sm"])
        else:
            ctrl.set_jt_goals(t, x[f"jt{t}.q"], x[f"jt{t}.dq"], x[f"jt{t}.ddq"])


_hip = None


def device_rows(g, which, task, rows):
    """rows [0, rows) of a ctx buffer (sai2b_device_buffer), copied to the host once the ctx stream is idle"""
    global _hip
    if _hip is None:
        _hip = C.CDLL(pkg._abi.LIB_PATH).hipMemcpy  # the HIP runtime the product library runs on
        _hip.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    g.synchronize()
    ptr = g.device_buffer(which, task)
    assert ptr, (which, task)
    out = np.empty((rows, g.B))
    assert _hip(out.ctypes.data, ptr, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def integrators(ctrl, tasks):
    """[per task: MotionForceTask [12][B] (position, orientation, force, moment), JointTask [k0][B]]"""
    out = []
    for t, (kind, _) in enumerate(tasks):
        rows = 12 if kind == "mft" else ctrl.tasks[t].task_dof
        if isinstance(ctrl, ol.Oracle):
            out.append(ctrl.get_mft_integrators(t) if kind == "mft" else ctrl.get_jt_integrators(t))
        else:
            out.append(device_rows(ctrl, pkg._abi.BUF_STATE, t, rows))
    return out
